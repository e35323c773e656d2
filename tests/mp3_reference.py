"""Independent NumPy MP3 for the tests: the unscaled terms (pp, hh, ring) of the restricted MP3 energy from a dense spherical
(mu nu|la si) tensor and canonical RHF orbitals (occupied window [n_frozen, n_occ), virtual window [n_occ, N)), in two forms:
  * spin_orbital_terms: the spin-orbital expressions of run_unrestricted_MP3 (tuna_mp.py:1524-1526) on the antisymmetrised
    <pq||rs> of the spin orbitals (p alpha, p beta) of the same spatial orbitals, D = e_i + e_j - e_a - e_b;
  * restricted_terms: the closed-shell expressions of run_restricted_MP3 (tuna_mp.py:1450-1470) in the MO basis, dense (ac|bd).
ao_direct_ladder is the particle-particle ladder the way the library forms it: T_ij = C_v t_ij C_v^T,
Z_ij[mu][nu] = sum (mu la|nu si) T_ij[la][si], X_pp[ij] = 1/2 C_v^T Z_ij C_v."""
from __future__ import annotations

import numpy as np

from ump2_reference import dense_eri  # noqa: F401  (re-exported for the tests)


def mo_tensor(E, C1, C2, C3, C4):
    """(pq|rs) = sum C1[mu,p] C2[nu,q] C3[la,r] C4[si,s] (mu nu|la si) -> [p, q, r, s]."""
    t = np.tensordot(E, C4, axes=(3, 0))
    t = np.tensordot(t, C3, axes=(2, 0))
    t = np.tensordot(t, C2, axes=(1, 0))
    t = np.tensordot(t, C1, axes=(0, 0))
    return np.ascontiguousarray(t.transpose(3, 2, 1, 0))


def _windows(C, eps, n_occ, n_frozen):
    C, eps = np.asarray(C, float), np.asarray(eps, float)
    return C[:, n_frozen:n_occ], C[:, n_occ:], eps[n_frozen:n_occ], eps[n_occ:]


def amplitudes(ovov, eo, ev):
    """t[i j a b] = (ia|jb) / D and t'[i j a b] = 2 [2 (ia|jb) - (ib|ja)] / D from ovov[i a j b] = (ia|jb)."""
    D = eo[:, None, None, None] - ev[None, :, None, None] + eo[None, None, :, None] - ev[None, None, None, :]
    t = (ovov / D).transpose(0, 2, 1, 3)
    tp = (2.0 * (2.0 * ovov - ovov.transpose(0, 3, 2, 1)) / D).transpose(0, 2, 1, 3)
    return np.ascontiguousarray(t), np.ascontiguousarray(tp)


def restricted_terms(E, C, eps, n_occ, n_frozen=0):
    """(E_pp, E_hh, E_ring) of E_MP3 = sum t'_ijab X_ijab in the MO basis."""
    Co, Cv, eo, ev = _windows(C, eps, n_occ, n_frozen)
    ovov = mo_tensor(E, Co, Cv, Co, Cv)
    oovv = mo_tensor(E, Co, Co, Cv, Cv)
    oooo = mo_tensor(E, Co, Co, Co, Co)
    vvvv = mo_tensor(E, Cv, Cv, Cv, Cv)
    t, tp = amplitudes(ovov, eo, ev)
    X_pp = 0.5 * np.einsum("ijcd,acbd->ijab", t, vvvv, optimize=True)
    X_hh = 0.5 * np.einsum("klab,kilj->ijab", t, oooo, optimize=True)
    # (bj|kc) = ovov[j b k c], (bc|kj) = oovv[k j b c], (bc|ki) = oovv[k i b c]
    X_ring = (np.einsum("ikac,jbkc->ijab", t, 2.0 * ovov, optimize=True) - np.einsum("ikac,kjbc->ijab", t, oovv, optimize=True)
              - np.einsum("kjac,kibc->ijab", t, oovv, optimize=True) - np.einsum("kiac,jbkc->ijab", t, ovov, optimize=True))
    return tuple(float(np.sum(tp * X)) for X in (X_pp, X_hh, X_ring))


def _so_block(g, r1, r2, r3, r4):
    """<PQ||RS> for the spin orbitals P = (p, spin) of the spatial index ranges r1..r4 (spin fastest), from the spatial (pq|rs) = g."""
    d = np.eye(2)

    def phys(a, b, c, e):                                  # <pq|rs> = (pr|qs)
        return g[np.ix_(a, c, b, e)].transpose(0, 2, 1, 3)
    A = np.einsum("pqrs,ac,bd->paqbrcsd", phys(r1, r2, r3, r4), d, d, optimize=True)
    A -= np.einsum("pqsr,ad,bc->paqbrcsd", phys(r1, r2, r4, r3), d, d, optimize=True)
    return A.reshape(2 * len(r1), 2 * len(r2), 2 * len(r3), 2 * len(r4))


def spin_orbital_terms(E, C, eps, n_occ, n_frozen=0, chunk=8):
    """(E_pp, E_hh, E_ring) of tuna_mp.py:1524-1526:
        pp   = 1/8 sum <ij||ab> <ab||cd> <cd||ij> / (D_ijab D_ijcd)
        hh   = 1/8 sum <ij||ab> <kl||ij> <ab||kl> / (D_ijab D_klab)
        ring =     sum <ij||ab> <kb||cj> <ac||ik> / (D_ijab D_ikac)
    <ab||cd> is formed a few virtuals at a time."""
    C, eps = np.asarray(C, float), np.asarray(eps, float)
    N = C.shape[0]
    g = mo_tensor(E, C, C, C, C)
    occ, vir = np.arange(n_frozen, n_occ), np.arange(n_occ, N)
    eo, ev = np.repeat(eps[occ], 2), np.repeat(eps[vir], 2)
    e = 1.0 / (eo[:, None, None, None] + eo[None, :, None, None] - ev[None, None, :, None] - ev[None, None, None, :])
    oovv, oooo = _so_block(g, occ, occ, vir, vir), _so_block(g, occ, occ, occ, occ)
    vvoo, ovvo = _so_block(g, vir, vir, occ, occ), _so_block(g, occ, vir, vir, occ)
    no, nv = 2 * len(occ), 2 * len(vir)
    A = (oovv * e).reshape(no * no, nv * nv)                 # <ij||ab> / D_ijab
    Y = (vvoo.transpose(2, 3, 0, 1) * e).reshape(no * no, nv * nv)   # <cd||ij> / D_ijcd  [ij][cd]
    M = A @ Y.T                                              # [ij][kl]: sum_ab <ij||ab> <ab||kl> / (D_ijab D_klab)
    hh = 0.125 * float(np.sum(oooo.reshape(no * no, no * no).T * M))
    pp = 0.0
    A3 = A.reshape(no * no, nv, nv)
    for a0 in range(0, len(vir), chunk):
        a1 = min(len(vir), a0 + chunk)
        blk = _so_block(g, vir[a0:a1], vir, vir, vir).reshape(2 * (a1 - a0) * nv, nv * nv)   # <ab||cd>, a in the slice
        pp += 0.125 * float(np.sum((A3[:, 2 * a0:2 * a1, :].reshape(no * no, -1) @ blk) * Y))
    ring = float(np.einsum("ijab,kbcj,acik,ikac->", oovv * e, ovvo, vvoo, e, optimize=True))
    return pp, hh, ring


def ao_direct_ladder(E, C, eps, n_occ, n_frozen=0):
    """(X_pp[i j a b] via the AO pair matrices, Z[i j mu nu]): the particle-particle ladder as the library forms it."""
    Co, Cv, eo, ev = _windows(C, eps, n_occ, n_frozen)
    t, _ = amplitudes(mo_tensor(E, Co, Cv, Co, Cv), eo, ev)
    T = np.einsum("la,ijab,sb->ijls", Cv, t, Cv, optimize=True)
    Z = np.einsum("mlns,ijls->ijmn", E, T, optimize=True)
    X = 0.5 * np.einsum("ma,ijmn,nb->ijab", Cv, Z, Cv, optimize=True)
    return X, Z


def mo_ladder(E, C, eps, n_occ, n_frozen=0):
    """X_pp[i j a b] = 1/2 sum_cd t_ijcd (ac|bd) with the dense MO block."""
    Co, Cv, eo, ev = _windows(C, eps, n_occ, n_frozen)
    t, _ = amplitudes(mo_tensor(E, Co, Cv, Co, Cv), eo, ev)
    return 0.5 * np.einsum("ijcd,acbd->ijab", t, mo_tensor(E, Cv, Cv, Cv, Cv), optimize=True)


def blocks_from_coulomb(J_of, Co, Cv, batch=64):
    """(oovv[i j a b] = (ij|ab), oooo[k i l j] = (ki|lj)) from Coulomb matrices: with D_ij = (c_i c_j^T + c_j c_i^T) / 2,
    J(D_ij)[la][si] = (la si|ij), so (ij|ab) = C_v^T J(D_ij) C_v and (ij|kl) = C_o^T J(D_ij) C_o.  J_of maps a batch of symmetric
    densities [n, N, N] to their Coulomb matrices; one density per pair i <= j."""
    o, v = Co.shape[1], Cv.shape[1]
    oovv, oooo = np.empty((o, o, v, v)), np.empty((o, o, o, o))
    pairs = [(i, j) for i in range(o) for j in range(i + 1)]
    for s in range(0, len(pairs), batch):
        chunk = pairs[s:s + batch]
        D = np.stack([0.5 * (np.outer(Co[:, i], Co[:, j]) + np.outer(Co[:, j], Co[:, i])) for i, j in chunk])
        J = np.asarray(J_of(D)).reshape(len(chunk), Co.shape[0], Co.shape[0])
        vv, oo = np.matmul(Cv.T, np.matmul(J, Cv)), np.matmul(Co.T, np.matmul(J, Co))
        for n, (i, j) in enumerate(chunk):
            oovv[i, j], oovv[j, i] = vv[n], vv[n]
            oooo[i, j], oooo[j, i] = oo[n], oo[n]
    return oovv, oooo


def terms_from_blocks(ovov, oovv, oooo, Z_of, Cv, eo, ev, batch=64):
    """((E_pp, E_hh, E_ring), (S_pp, S_hh, S_ring)): the expressions of restricted_terms from the blocks ovov[i a j b] = (ia|jb),
    oovv[i j a b] = (ij|ab), oooo[k i l j] = (ki|lj) and a callback Z_of that maps a batch of AO matrices T [n, N, N] to
    Z[T][mu][nu] = sum (mu la|nu si) T[la][si]; never forms (ac|bd).  S = sum |t'_ijab X_ijab| per term: the yardstick of an error in the
    term, which cancellation inside the sum cannot shrink.  The hole-hole and ring contractions are explicit reshaped GEMMs (BLAS)."""
    o, v = len(eo), len(ev)
    ov = o * v
    t, tp = amplitudes(ovov, eo, ev)                                # [i j a b]
    # particle-particle ladder: T_ij = C_v t_ij C_v^T, X_ij = 1/2 C_v^T Z_ij C_v
    tf = t.reshape(o * o, v, v)
    X_pp = np.empty((o * o, v, v))
    for s in range(0, o * o, batch):
        T = np.matmul(Cv, np.matmul(tf[s:s + batch], Cv.T))
        Z = np.asarray(Z_of(T)).reshape(T.shape)
        X_pp[s:s + batch] = 0.5 * np.matmul(Cv.T, np.matmul(Z, Cv))
    X_pp = X_pp.reshape(o, o, v, v)
    # hole-hole ladder: X[(ij)][(ab)] = 1/2 sum_(kl) (ki|lj) t[(kl)][(ab)]
    M = np.ascontiguousarray(oooo.transpose(1, 3, 0, 2)).reshape(o * o, o * o)
    X_hh = (0.5 * (M @ t.reshape(o * o, v * v))).reshape(o, o, v, v)
    # ring: with A[(ia)][(kc)] = t_ikac, A'[(ja)][(kc)] = t_kjac, G[(kc)][(jb)] = (kc|jb), H[(kc)][(jb)] = (kj|bc):
    #   X_ijab = [A (2 G - H)][(ia)][(jb)] - [A' H][(ja)][(ib)] - [A' G][(ia)][(jb)]
    A = np.ascontiguousarray(t.transpose(0, 2, 1, 3)).reshape(ov, ov)
    A2 = np.ascontiguousarray(t.transpose(1, 2, 0, 3)).reshape(ov, ov)
    G = np.ascontiguousarray(ovov).reshape(ov, ov)
    H = np.ascontiguousarray(oovv.transpose(0, 3, 1, 2)).reshape(ov, ov)
    R = A @ (2.0 * G - H) - A2 @ G                                  # [(ia)][(jb)]
    R2 = A2 @ H                                                     # [(ja)][(ib)]
    X_ring = R.reshape(o, v, o, v).transpose(0, 2, 1, 3) - R2.reshape(o, v, o, v).transpose(2, 0, 1, 3)
    E = tuple(float(np.sum(tp * X)) for X in (X_pp, X_hh, X_ring))
    S = tuple(float(np.sum(np.abs(tp * X))) for X in (X_pp, X_hh, X_ring))
    return E, S
