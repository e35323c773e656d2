"""Independent NumPy CIS(D) for the tests (no library code): the doubles correction of Head-Gordon, Rico, Oumi and Lee, Chem. Phys.
Lett. 219, 21 (1994), in SPIN orbitals on antisymmetrised integrals <pq||rs> = <pq|rs> - <pq|sr>, <pq|rs> = (pr|qs), from a dense
spherical (mu nu|la si) tensor and canonical RHF orbitals (occupied window [n_frozen, n_occ), virtual window [n_occ, N)).  With
Delta_ijab = e_a + e_b - e_i - e_j, a_ijab = -<ij||ab> / Delta_ijab (the MP2 amplitudes) and a normalised state b_ia of energy w:
    u_ijab = sum_c (<ab||cj> b_ic - <ab||ci> b_jc) + sum_k (<ka||ij> b_kb - <kb||ij> b_ka)
    v_ia   = 1/2 sum_jkbc <jk||bc> (b_ib a_jkca + b_ja a_ikcb + 2 b_jb a_ikac)
    E_direct = -1/4 sum_ijab u_ijab^2 / (Delta_ijab - w),   E_indirect = sum_ia b_ia v_ia,   E_D = E_direct + E_indirect
A spin orbital is (spin, spatial orbital), alpha first.  A closed-shell singlet has b_alpha = b_beta = b / sqrt(2), the M_S = 0 triplet
b_alpha = -b_beta = b / sqrt(2), b the spatial vector [o, v] the library takes.  Nothing is spin-adapted here: the library's
restricted expressions are a different route to the same number.  Meant for small systems: the <ab||cj> block has (2 v)^3 (2 o)
values."""
from __future__ import annotations

import numpy as np

from mp3_reference import _windows, dense_eri, mo_tensor  # noqa: F401  (dense_eri re-exported for the tests)


def _spin_block(E, P, Q, R, S):
    """<pq|rs> over spin orbitals [2 np, 2 nq, 2 nr, 2 ns] for spatial coefficient matrices P, Q, R, S: (pr|qs), spins of p and r alike
    and spins of q and s alike."""
    sp = mo_tensor(E, P, R, Q, S).transpose(0, 2, 1, 3)       # [p q r s] = (pr|qs)
    n = sp.shape
    out = np.zeros((2, n[0], 2, n[1], 2, n[2], 2, n[3]))
    for s1 in range(2):
        for s2 in range(2):
            out[s1, :, s2, :, s1, :, s2, :] = sp
    return out.reshape(2 * n[0], 2 * n[1], 2 * n[2], 2 * n[3])


def prepare(E, C, eps, n_occ, n_frozen=0):
    """The state-independent pieces: {"vvvo", "ovoo", "oovv"} antisymmetrised, "a" the MP2 amplitudes, "Delta", "o", "v"}."""
    Co, Cv, eo, ev = _windows(C, eps, n_occ, n_frozen)
    o, v = Co.shape[1], Cv.shape[1]
    vvvo = _spin_block(E, Cv, Cv, Cv, Co) - _spin_block(E, Cv, Cv, Co, Cv).transpose(0, 1, 3, 2)
    ovoo = _spin_block(E, Co, Cv, Co, Co)
    ovoo = ovoo - ovoo.transpose(0, 1, 3, 2)
    oovv = _spin_block(E, Co, Co, Cv, Cv)
    oovv = oovv - oovv.transpose(0, 1, 3, 2)
    so, sv = np.concatenate([eo, eo]), np.concatenate([ev, ev])
    Delta = sv[None, None, :, None] + sv[None, None, None, :] - so[:, None, None, None] - so[None, :, None, None]
    return dict(vvvo=vvvo, ovoo=ovoo, oovv=oovv, a=-oovv / Delta, Delta=Delta, o=o, v=v)


def working_equations(E, C, eps, n_occ, n_frozen, b, omega, triplet):
    """(E_direct, E_indirect) by the spin-adapted expressions the library evaluates (tf_cisd.hip.h), in NumPy on spatial orbitals and
    with no block of three virtual indices: the half-dressed block M[iajb] = (i~ a|jb) - sum_k b_ka (ki|jb) for the direct part, L, t,
    2 t - t', Goo and Gvv for the indirect part."""
    Co, Cv, eo, ev = _windows(C, eps, n_occ, n_frozen)
    b = np.asarray(b, float).reshape(Co.shape[1], Cv.shape[1])
    g = mo_tensor(E, Co, Cv, Co, Cv)                          # [i a j b]
    M = mo_tensor(E, Cv @ b.T, Cv, Co, Cv) - np.einsum("ka,kijb->iajb", b, mo_tensor(E, Co, Co, Co, Cv), optimize=True)
    D = eo[:, None, None, None] - ev[None, :, None, None] + eo[None, None, :, None] - ev[None, None, None, :]      # [i a j b]
    s = 1.0 / (D + omega)
    uS = M + M.transpose(2, 3, 0, 1)
    uT = M - M.transpose(2, 3, 0, 1)
    uSx = uS.transpose(2, 1, 0, 3)                            # u_S[jiab]
    E_direct = np.sum(s * uS * (uS - 0.5 * uSx)) if not triplet else 0.5 * np.sum(s * (uS * uS - uS * uSx + uT * uT))
    t = g / D
    L, tt = 2 * g - g.transpose(0, 3, 2, 1), 2 * t - t.transpose(0, 3, 2, 1)
    Goo = np.einsum("jbkc,ibkc->ij", L, t, optimize=True)
    Gvv = np.einsum("jbkc,jakc->ba", L, t, optimize=True)
    if not triplet:
        y = np.einsum("iakc,kc->ia", tt, np.einsum("kcjb,jb->kc", L, b, optimize=True), optimize=True)
    else:
        y = np.einsum("icka,kc->ia", t, np.einsum("jckb,jb->kc", g, b, optimize=True), optimize=True)
    E_indirect = np.sum(b * y) - np.einsum("ia,ja,ij->", b, b, Goo, optimize=True) - np.einsum("ia,ib,ba->", b, b, Gvv, optimize=True)
    return float(E_direct), float(E_indirect)


def correction(prep, b, omega, triplet):
    """{"E_direct", "E_indirect", "E_D", "min_denominator", "S_direct", "S_indirect"} of one state: b [o, v] spatial and normalised, omega
    its energy, triplet 0 or 1.  S_* = the sum of the magnitudes of the terms of each part (the scale of its rounding error)."""
    o, v = prep["o"], prep["v"]
    b = np.asarray(b, float).reshape(o, v) / np.sqrt(2.0)
    bs = np.zeros((2, o, 2, v))
    bs[0, :, 0, :] = b
    bs[1, :, 1, :] = -b if triplet else b
    bs = bs.reshape(2 * o, 2 * v)
    vvvo, ovoo, oovv, a, Delta = (prep[k] for k in ("vvvo", "ovoo", "oovv", "a", "Delta"))
    u = np.einsum("abcj,ic->ijab", vvvo, bs, optimize=True)
    u = u - u.transpose(1, 0, 2, 3)
    h = np.einsum("kaij,kb->ijab", ovoo, bs, optimize=True)
    u = u + h - h.transpose(0, 1, 3, 2)
    den = Delta - omega
    terms = -0.25 * u * u / den
    v1 = 0.5 * np.einsum("jkbc,ib,jkca->ia", oovv, bs, a, optimize=True)
    v2 = 0.5 * np.einsum("jkbc,ja,ikcb->ia", oovv, bs, a, optimize=True)
    v3 = np.einsum("jkbc,jb,ikac->ia", oovv, bs, a, optimize=True)
    E_direct, E_indirect = float(terms.sum()), float(np.sum(bs * (v1 + v2 + v3)))
    S_indirect = float(np.sum(np.abs(bs * v1)) + np.sum(np.abs(bs * v2)) + np.sum(np.abs(bs * v3)))
    return dict(E_direct=E_direct, E_indirect=E_indirect, E_D=E_direct + E_indirect, min_denominator=float(np.abs(den).min()),
                S_direct=float(np.abs(terms).sum()), S_indirect=S_indirect)
