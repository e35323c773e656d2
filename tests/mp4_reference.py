"""Independent NumPy MP4(SDQ) for the tests: the singles, doubles and quadruples components of the fourth-order energy from a dense
spherical (mu nu|la si) tensor and canonical RHF orbitals (occupied window [n_frozen, n_occ), virtual window [n_occ, N)).  No formula
of the library's MP4 appears here; the components are differences of undamped coupled-cluster steps from the MP2 guess, in spin
orbitals (ccd_reference.spin_orbital_iterations and a spin-orbital LCCSD step written below):
    E_D = E[LCCD step 2] - E[LCCD step 1]      (the second step's amplitudes are t + t2: one more application of the linear terms)
    E_Q = E[CCD step 1]  - E[LCCD step 1]      (the terms quadratic in t, evaluated on the first-order amplitudes)
    E_S = E[LCCSD step 2] - E[LCCD step 2]     (the singles an LCCSD step 1 leaves, fed into the doubles equation of step 2)
With canonical orbitals step 1 of LCCSD has the doubles of LCCD and the second-order singles
    t_ia = -1/2 [ sum_kcd <ka||cd> t_ikcd + sum_klc <kl||ic> t_klac ] / (e_i - e_a),
and step 2 adds  P(ij) sum_c t_ic <ab||cj> - P(ab) sum_k t_ka <kb||ij>  to the doubles residual (Shavitt and Bartlett, Many-Body Methods
in Chemistry and Physics, the terms of eqs. 9.125 and 9.126 linear in the amplitudes); E = 1/4 sum <ij||ab> t_ijab.
singles_hermitian is the same E_S as the quadratic form sum_ia (e_i - e_a) t_ia^2, a check of the checker."""
from __future__ import annotations

import numpy as np

import ccd_reference as ccr
from mp3_reference import _so_block, mo_tensor


def _so(E, C, eps, n_occ, n_frozen):
    C, eps = np.asarray(C, float), np.asarray(eps, float)
    N = C.shape[0]
    g = mo_tensor(E, C, C, C, C)
    occ, vir = np.arange(n_frozen, n_occ), np.arange(n_occ, N)
    return g, occ, vir, np.repeat(eps[occ], 2), np.repeat(eps[vir], 2)


def singles_amplitudes(E, C, eps, n_occ, n_frozen=0):
    """(t1[i a] in spin orbitals, t[i j a b] first-order doubles in spin orbitals, the blocks used)."""
    g, occ, vir, eo, ev = _so(E, C, eps, n_occ, n_frozen)
    oovv, ovvv, ooov = _so_block(g, occ, occ, vir, vir), _so_block(g, occ, vir, vir, vir), _so_block(g, occ, occ, occ, vir)
    D2 = eo[:, None, None, None] + eo[None, :, None, None] - ev[None, None, :, None] - ev[None, None, None, :]
    t = oovv / D2
    w = -0.5 * np.einsum("kacd,ikcd->ia", ovvv, t, optimize=True) - 0.5 * np.einsum("klic,klac->ia", ooov, t, optimize=True)
    return w / (eo[:, None] - ev[None, :]), t, (g, occ, vir, eo, ev, oovv, D2)


def singles_energy(E, C, eps, n_occ, n_frozen=0):
    """E[LCCSD step 2] - E[LCCD step 2]: the doubles that the second-order singles drive, contracted with <ij||ab>."""
    t1, _, (g, occ, vir, eo, ev, oovv, D2) = singles_amplitudes(E, C, eps, n_occ, n_frozen)
    vvvo, ovoo = _so_block(g, vir, vir, vir, occ), _so_block(g, occ, vir, occ, occ)
    A = np.einsum("ic,abcj->ijab", t1, vvvo, optimize=True)
    B = np.einsum("ka,kbij->ijab", t1, ovoo, optimize=True)
    dR = (A - A.transpose(1, 0, 2, 3)) - (B - B.transpose(0, 1, 3, 2))
    return 0.25 * float(np.sum(oovv * dR / D2))


def singles_hermitian(E, C, eps, n_occ, n_frozen=0):
    t1, _, (g, occ, vir, eo, ev, oovv, D2) = singles_amplitudes(E, C, eps, n_occ, n_frozen)
    return float(np.sum((eo[:, None] - ev[None, :]) * t1 * t1))


def components(E, C, eps, n_occ, n_frozen=0, level="SDQ", form="spin_orbital"):
    """{"E_S", "E_D", "E_Q", "E_MP4", "E_MP2", "E_MP3"} of MP4(SDQ), or MP4(DQ) (E_S = 0.0).  form "restricted" takes the steps of E_D
    and E_Q from ccd_reference.restricted_iterations (the closed-shell equations with the dense (ac|bd): the larger systems, where the
    spin-orbital <ab||cd> does not fit); the singles are always the spin-orbital ones."""
    steps = {"spin_orbital": ccr.spin_orbital_iterations, "restricted": ccr.restricted_iterations}[form]
    lccd = steps(E, C, eps, n_occ, n_frozen, "LCCD", 2)["energies"]
    r = steps(E, C, eps, n_occ, n_frozen, "CCD", 1)
    E_D, E_Q = lccd[1] - lccd[0], r["energies"][0] - lccd[0]
    if level == "SDQ":
        E_S = singles_energy(E, C, eps, n_occ, n_frozen)
    elif level == "DQ":
        E_S = 0.0
    else:
        raise ValueError(level)
    return {"E_S": E_S, "E_D": E_D, "E_Q": E_Q, "E_MP4": E_S + E_D + E_Q, "E_MP2": r["E_MP2"], "E_MP3": lccd[0] - r["E_MP2"]}


def occupied_rows(ovov, Z_of, Co, Cv, eo, ev, batch=64):
    """(t[i j a b], OV[i j k a] = [C_o^T Z[C_v t_ij C_v^T] C_v]_ka = sum_cd (kc|ad) t_ijcd) from ovov[i a j b] = (ia|jb) and a callback Z_of
    that maps a batch of AO matrices T [n, N, N] to Z[T][mu][nu] = sum (mu la|nu si) T[la][si]."""
    from mp3_reference import amplitudes
    o, v = len(eo), len(ev)
    t, _ = amplitudes(ovov, eo, ev)
    tf = t.reshape(o * o, v, v)
    OV = np.empty((o * o, o, v))
    for s in range(0, o * o, batch):
        T = np.matmul(Cv, np.matmul(tf[s:s + batch], Cv.T))
        Z = np.asarray(Z_of(T)).reshape(T.shape)
        OV[s:s + batch] = np.matmul(Co.T, np.matmul(Z, Cv))
    return t, OV.reshape(o, o, o, v)


def singles_from_rows(t, OV, q, eo, ev):
    """(E_S, S) in the closed-shell form from occupied_rows' t and OV and q[k i l d] = (ki|ld); never forms an integral with three virtual
    indices.  With L_pqrs = 2 (pq|rs) - (ps|rq):
        u_ia = sum_kld t_klad L_kild - sum_k (2 OV_ki - OV_ik)[k a],   t1 = -u / (e_i - e_a),   E_S = 2 sum_ia (e_i - e_a) t1_ia^2
    (the Hermitian form: two spins of one spatial amplitude).  S = 2 sum_ia |t1_ia| (|sum_kld t_klad L_kild| + |sum_k (2 OV_ki - OV_ik)[k a]|):
    the yardstick of an error in the term, which the cancellation between the two parts of u cannot shrink.  A frozen core is a slice of
    every argument."""
    L = 2.0 * q - q.transpose(2, 1, 0, 3)                            # [k i l d] = 2 (ki|ld) - (kd|li)
    u1 = np.einsum("klad,kild->ia", t, L, optimize=True)
    u2 = 2.0 * np.einsum("kika->ia", OV) - np.einsum("ikka->ia", OV)
    de = eo[:, None] - ev[None, :]
    t1 = -(u1 - u2) / de
    return 2.0 * float(np.sum(de * t1 * t1)), 2.0 * float(np.sum(np.abs(t1) * (np.abs(u1) + np.abs(u2))))


def singles_from_blocks(ovov, q, Z_of, Co, Cv, eo, ev, batch=64):
    """singles_from_rows of occupied_rows"""
    t, OV = occupied_rows(ovov, Z_of, Co, Cv, eo, ev, batch)
    return singles_from_rows(t, OV, q, eo, ev)
