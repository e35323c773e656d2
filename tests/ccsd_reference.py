"""Independent NumPy LCCSD / QCISD / CCSD for the tests: the singles-and-doubles amplitude iteration from canonical RHF orbitals
(windows, D and the guess t2 of ccd_reference.py; t1 starts at zero, D_ia = e_i - e_a), E = sum [2 (ia|jb) - (ib|ja)] (t_ijab + t_ia t_jb)
with the t_ia t_jb part (the disconnected energy) kept by CCSD alone, in three forms:
  * spin_orbital_iterations: the textbook spin-orbital equations (Stanton, Gauss, Watts, Bartlett, J. Chem. Phys. 94, 4334, eqs. 1-13,
    canonical orbitals) on the antisymmetrised <pq||rs>; QCISD keeps, beside everything linear, the t2 t2 terms of the doubles and the
    t1 t2 terms of the singles; LCCSD keeps the linear terms.  The alpha-beta block of t2 and the alpha block of t1 are the closed-shell
    amplitudes;
  * restricted_iterations: the closed-shell equations in chemists' notation on dense MO blocks, (ac|bd) and (ia|bc) included;
  * iterations_from_blocks: the closed-shell equations staged as the library stages them, nothing with three virtual indices:
      - dressed pair matrices T_ij = C_v th_ij C_v^T + c_i b_j^T + b_i c_j^T with b_i = C_v t_i (th = t2, CCSD: t2 + t1 t1), one batch loop
        of the callback Z_of per step, Z_ij[mu][nu] = sum (mu la|nu si) T_ij[la][si];
      - the blocks of the back-transformation: vv = C_v^T Z_ij C_v (the ladder and sum_c (ia|cb) t_jc with its image), ov = C_o^T Z_ij C_v
        (the three-virtual terms of the singles, and CCSD's t1 parts of W_cdab, -(ik|cb) t_ka t_jc and -(ia|ck) t_jc t_kb);
      - CCSD's dressed o^2 v^2 blocks from a callback mo_of(C1, C2, C3, C4): W_icak's t1 part (L_i X_a|kc) and W_ciak's (L_i k|X_a c),
        L = C_o + C_v t1^T, X = C_v - C_o t1, and its M = 2 J - K of the density C_o t1 C_v^T from a callback jk_of (the t1 parts of
        L_ca and L_ik);
      - the blocks (ia|jb), (ij|ab), (ik|jl), (ik|ja) and GEMMs.
All three pack (t2, t1) into one vector (t1 behind t2) and run ccd_reference.iterate on it: the DIIS error vector is the concatenation,
damping applies to both, and convergence needs |dE|, ||dt2||_2 and ||dt1||_2 under their thresholds.  Each returns {"t1", "t2",
"energies", "n_iter", "converged", "E_MP2", "E_connected", "E_disconnected", "dt1_norm"} of the last step taken."""
from __future__ import annotations

import numpy as np

from ccd_reference import _denominators, iterate
from mp3_reference import _so_block, _windows, mo_tensor

METHODS = ("LCCSD", "QCISD", "CCSD")


def _check(method):
    if method not in METHODS:
        raise ValueError(method)


def _run(step, energy_parts, t2_0, shape1, method, k, **loop):
    """ccd_reference.iterate on the packed vector; step(t1, t2) -> (t1_new, t2_new)."""
    n2 = t2_0.size

    def unpack(x):
        return x[n2:].reshape(shape1), x[:n2].reshape(t2_0.shape)

    def pack(t1, t2):
        return np.concatenate([t2.ravel(), t1.ravel()])

    def total(x):
        c, d = energy_parts(*unpack(x))
        return c + (d if method == "CCSD" else 0.0)
    r = iterate(lambda x: pack(*step(*unpack(x))), total, pack(np.zeros(shape1), t2_0), k,
                norm=lambda d: max(float(np.linalg.norm(d[:n2])), float(np.linalg.norm(d[n2:]))), **loop)
    t1, t2 = unpack(r["t"])
    c, d = energy_parts(t1, t2)
    return {"t1": t1.copy(), "t2": t2.copy(), "energies": r["energies"], "n_iter": r["n_iter"], "converged": r["converged"],
            "E_connected": float(c), "E_disconnected": float(d) if method == "CCSD" else 0.0, "E_MP2": float(energy_parts(np.zeros(shape1), t2_0)[0])}


def _energy_parts(ovov):
    w = (2.0 * ovov - ovov.transpose(0, 3, 2, 1)).transpose(0, 2, 1, 3)       # [i j a b]: 2 (ia|jb) - (ib|ja)
    return lambda t1, t2: (np.sum(w * t2), np.einsum("ijab,ia,jb->", w, t1, t1, optimize=True))


def restricted_step(ovov, oovv, oooo, ooov, ovvv, vvvv, eo, ev, method):
    """(t1, t2) -> (t1_new, t2_new).  ovov[i a j b] = (ia|jb), oovv[i j a b] = (ij|ab), oooo[i k j l] = (ik|jl), ooov[i k j a] = (ik|ja),
    ovvv[i a b c] = (ia|bc), vvvv[a c b d] = (ac|bd)."""
    _check(method)
    es = np.einsum
    D2, D1 = _denominators(eo, ev), eo[:, None] - ev[None, :]
    g = ovov.transpose(0, 2, 1, 3)
    w = 2.0 * ovov - ovov.transpose(0, 3, 2, 1)                               # [k c l d] = 2 (kc|ld) - (kd|lc)
    full, quad = method == "CCSD", method != "LCCSD"

    def step(t1, t2):
        th = t2 + es("ia,jb->ijab", t1, t1) if full else t2
        # ---- singles
        s = 2.0 * es("kdac,ikcd->ia", ovvv, th, optimize=True) - es("kcad,ikcd->ia", ovvv, th, optimize=True)
        s += -2.0 * es("iklc,klac->ia", ooov, th, optimize=True) + es("ilkc,klac->ia", ooov, th, optimize=True)
        s += 2.0 * es("iakc,kc->ia", ovov, t1, optimize=True) - es("ikac,kc->ia", oovv, t1, optimize=True)
        F_ik = F_ca = None
        if quad:
            F_ik = es("kcld,ilcd->ik", w, th, optimize=True)
            F_ca = -es("kcld,klad->ca", w, th, optimize=True)
            F_kc = es("kcld,ld->kc", w, t1, optimize=True)
            s += es("ca,ic->ia", F_ca, t1) - es("ik,ka->ia", F_ik, t1) + es("kc,kica->ia", F_kc, 2.0 * t2 - t2.transpose(1, 0, 2, 3), optimize=True)
            if full:
                s += es("kc,ic,ka->ia", F_kc, t1, t1, optimize=True)
        # ---- doubles
        Wo = oooo.transpose(0, 2, 1, 3)                                       # [i j k l] = (ik|jl)
        V = vvvv
        W1, W2 = ovov, oovv.transpose(0, 2, 1, 3)                             # [i a k c]: (ia|kc), (ik|ac)
        R = 0.5 * g
        if quad:
            Wo = Wo + es("kcld,ijcd->ijkl", ovov, th, optimize=True)
            W1 = W1 - 0.5 * es("ldkc,ilda->iakc", ovov, t2, optimize=True) + 0.5 * es("ldkc,ilad->iakc", w, t2, optimize=True)
            W2 = W2 - 0.5 * es("lckd,ilda->iakc", ovov, t2, optimize=True)
            L_ca, L_ik = F_ca, F_ik
            if full:
                P = es("jlkc,ic->ijkl", ooov, t1, optimize=True)
                Wo = Wo + P + P.transpose(1, 0, 3, 2)
                V = V - es("kdac,kb->acbd", ovvv, t1, optimize=True) - es("kcbd,ka->acbd", ovvv, t1, optimize=True)
                W1 = (W1 - es("ilkc,la->iakc", ooov, t1, optimize=True) + es("kcda,id->iakc", ovvv, t1, optimize=True)
                      - es("ldkc,id,la->iakc", ovov, t1, t1, optimize=True))
                W2 = (W2 - es("iklc,la->iakc", ooov, t1, optimize=True) + es("kdca,id->iakc", ovvv, t1, optimize=True)
                      - es("lckd,id,la->iakc", ovov, t1, t1, optimize=True))
                L_ca = F_ca + 2.0 * es("kdca,kd->ca", ovvv, t1, optimize=True) - es("kcda,kd->ca", ovvv, t1, optimize=True)
                L_ik = F_ik + 2.0 * es("iklc,lc->ik", ooov, t1, optimize=True) - es("ilkc,lc->ik", ooov, t1, optimize=True)
                R = R - es("ikcb,ka,jc->ijab", oovv, t1, t1, optimize=True) - es("iakc,jc,kb->ijab", ovov, t1, t1, optimize=True)
            R = R + es("ca,ijcb->ijab", L_ca, t2, optimize=True) - es("ik,kjab->ijab", L_ik, t2, optimize=True)
        R = R + 0.5 * es("ijkl,klab->ijab", Wo, th, optimize=True) + 0.5 * es("acbd,ijcd->ijab", V, th, optimize=True)
        R = R + es("iacb,jc->ijab", ovvv, t1, optimize=True) - es("jkia,kb->ijab", ooov, t1, optimize=True)
        R = R + es("iakc,kjcb->ijab", 2.0 * W1 - W2, t2, optimize=True) - es("iakc,kjbc->ijab", W1, t2, optimize=True)
        R = R - es("ibkc,kjac->ijab", W2, t2, optimize=True)
        return s / D1, (R + R.transpose(1, 0, 3, 2)) / D2
    return step


def restricted_iterations(E, C, eps, n_occ, n_frozen, method, k, **loop):
    Co, Cv, eo, ev = _windows(C, eps, n_occ, n_frozen)
    ovov, oovv, oooo = mo_tensor(E, Co, Cv, Co, Cv), mo_tensor(E, Co, Co, Cv, Cv), mo_tensor(E, Co, Co, Co, Co)
    ooov, ovvv, vvvv = mo_tensor(E, Co, Co, Co, Cv), mo_tensor(E, Co, Cv, Cv, Cv), mo_tensor(E, Cv, Cv, Cv, Cv)
    t0 = ovov.transpose(0, 2, 1, 3) / _denominators(eo, ev)
    return _run(restricted_step(ovov, oovv, oooo, ooov, ovvv, vvvv, eo, ev, method), _energy_parts(ovov), t0, (len(eo), len(ev)), method, k, **loop)


def spin_orbital_iterations(E, C, eps, n_occ, n_frozen, method, k, **loop):
    """Stanton et al.'s equations with f diagonal.  Returns the closed-shell blocks as "t1", "t2" and the full arrays as "t1_so", "t2_so";
    the norms of the convergence test are taken over those blocks, as the restricted iteration takes them."""
    _check(method)
    C, eps = np.asarray(C, float), np.asarray(eps, float)
    N = C.shape[0]
    g = mo_tensor(E, C, C, C, C)
    occ, vir = np.arange(n_frozen, n_occ), np.arange(n_occ, N)
    eo, ev = np.repeat(eps[occ], 2), np.repeat(eps[vir], 2)
    D2, D1 = _denominators(eo, ev), eo[:, None] - ev[None, :]
    oovv, oooo, vvvv = _so_block(g, occ, occ, vir, vir), _so_block(g, occ, occ, occ, occ), _so_block(g, vir, vir, vir, vir)
    ovvo, ooov, ovvv = _so_block(g, occ, vir, vir, occ), _so_block(g, occ, occ, occ, vir), _so_block(g, occ, vir, vir, vir)
    es = np.einsum
    full, quad = method == "CCSD", method != "LCCSD"
    no, nv = len(eo), len(ev)

    def P(X, ax1, ax2):
        return X - X.swapaxes(ax1, ax2)

    def step(t1, t2):
        tt = es("ia,jb->ijab", t1, t1)
        pair = P(tt, 2, 3) if full else 0.0 * t2
        tau, taus = t2 + pair, t2 + 0.5 * pair
        Fae, Fmi, Fme = np.zeros((nv, nv)), np.zeros((no, no)), np.zeros((no, nv))
        if quad:
            Fae = -0.5 * es("mnaf,mnef->ae", taus, oovv, optimize=True)
            Fmi = 0.5 * es("inef,mnef->mi", taus, oovv, optimize=True)
            Fme = es("nf,mnef->me", t1, oovv, optimize=True)
        Wmnij, Wabef, Wmbej = oooo, vvvv, ovvo
        if quad:
            Wmnij = Wmnij + 0.25 * es("ijef,mnef->mnij", tau, oovv, optimize=True)
            Wabef = Wabef + 0.25 * es("mnab,mnef->abef", tau, oovv, optimize=True)
            Wmbej = Wmbej - es("jnfb,mnef->mbej", 0.5 * t2 + (tt if full else 0.0 * t2), oovv, optimize=True)
        if full:
            Fae = Fae + es("mf,mafe->ae", t1, ovvv, optimize=True)
            Fmi = Fmi + es("ne,mnie->mi", t1, ooov, optimize=True)
            Wmnij = Wmnij + P(es("je,mnie->mnij", t1, ooov, optimize=True), 2, 3)
            Wabef = Wabef + P(es("mb,maef->abef", t1, ovvv, optimize=True), 0, 1)                  # <am||ef> = -<ma||ef>
            # <mb||ef> = ovvv;  <mn||ej> = -ooov[m n j e]
            Wmbej = Wmbej + es("jf,mbef->mbej", t1, ovvv, optimize=True) + es("nb,mnje->mbej", t1, ooov, optimize=True)
        # singles, with the blocks at hand: <na||if> = -ovvo[n a f i], <nm||ei> = -ooov[n m i e]
        s = es("nf,nafi->ia", t1, ovvo, optimize=True) - 0.5 * es("imef,maef->ia", t2, ovvv, optimize=True)
        s -= 0.5 * es("mnae,nmie->ia", t2, -ooov, optimize=True)                                   # <nm||ei> = -<nm||ie>
        s += es("ie,ae->ia", t1, Fae) - es("ma,mi->ia", t1, Fmi) + es("imae,me->ia", t2, Fme, optimize=True)
        # doubles
        R = oovv + 0.5 * es("mnab,mnij->ijab", tau, Wmnij, optimize=True) + 0.5 * es("ijef,abef->ijab", tau, Wabef, optimize=True)
        Fb = Fae - (0.5 * es("mb,me->be", t1, Fme) if full else 0.0)
        Fj = Fmi + (0.5 * es("je,me->mj", t1, Fme) if full else 0.0)
        if quad:
            R = R + P(es("ijae,be->ijab", t2, Fb, optimize=True), 2, 3) - P(es("imab,mj->ijab", t2, Fj, optimize=True), 0, 1)
        X = es("imae,mbej->ijab", t2, Wmbej, optimize=True)
        if full:
            X = X - es("ie,ma,mbej->ijab", t1, t1, ovvo, optimize=True)
        R = R + P(P(X, 0, 1), 2, 3)
        # P(ij) t_ie <ab||ej>, <ab||ej> = <ej||ab> = ovvv[j e b a]
        R = R + P(es("ie,jeba->ijab", t1, ovvv, optimize=True), 0, 1)
        # -P(ab) t_ma <mb||ij> = -P(ab) t_ma <ij||mb> = -P(ab) t_ma ooov[i j m b]
        R = R - P(es("ma,ijmb->ijab", t1, ooov, optimize=True), 2, 3)
        return s / D1, R / D2
    n2 = oovv.size

    def ab2(x):
        return x[0::2, 1::2, 0::2, 1::2]

    def energy_parts(t1, t2):
        return 0.25 * np.sum(oovv * t2), 0.5 * es("ijab,ia,jb->", oovv, t1, t1, optimize=True)

    def total(x):
        c, d = energy_parts(x[n2:].reshape(no, nv), x[:n2].reshape(oovv.shape))
        return c + (d if full else 0.0)

    def packed_step(x):
        t1, t2 = step(x[n2:].reshape(no, nv), x[:n2].reshape(oovv.shape))
        return np.concatenate([t2.ravel(), t1.ravel()])

    def norm(d):
        return max(float(np.linalg.norm(ab2(d[:n2].reshape(oovv.shape)))), float(np.linalg.norm(d[n2:].reshape(no, nv)[0::2, 0::2])))
    t0 = oovv / D2
    r = iterate(packed_step, total, np.concatenate([t0.ravel(), np.zeros(no * nv)]), k, norm=norm, **loop)
    t1, t2 = r["t"][n2:].reshape(no, nv), r["t"][:n2].reshape(oovv.shape)
    c, d = energy_parts(t1, t2)
    return {"t1": np.ascontiguousarray(t1[0::2, 0::2]), "t2": np.ascontiguousarray(ab2(t2)), "t1_so": t1, "t2_so": t2, "energies": r["energies"],
            "n_iter": r["n_iter"], "converged": r["converged"], "E_connected": float(c), "E_disconnected": float(d) if full else 0.0,
            "E_MP2": float(0.25 * np.sum(oovv * t0))}


def iterations_from_blocks(ovov, oovv, oooo, ooov, Z_of, mo_of, jk_of, Co, Cv, eo, ev, method, k, batch=64, counts=None, **loop):
    """ovov[i a j b] = (ia|jb), oovv[i j a b] = (ij|ab), oooo[i k j l] = (ik|jl), ooov[i k j a] = (ik|ja).  Z_of maps a batch of AO
    matrices to Z; mo_of(C1, C2, C3, C4)[p q r s] = (pq|rs); jk_of(Dm) = (J, K) with J[mu][nu] = sum (mu nu|la si) Dm[la][si],
    K[mu][nu] = sum (mu la|si nu) Dm[la][si].  counts (a dict) collects "Z_of" (calls), "loops" (batch loops), "mo_of", "jk_of"."""
    _check(method)
    counts = counts if counts is not None else {}
    for key in ("Z_of", "loops", "mo_of", "jk_of"):
        counts.setdefault(key, 0)
    o, v = len(eo), len(ev)
    ov = o * v
    D2, D1 = _denominators(eo, ev), eo[:, None] - ev[None, :]
    G = np.ascontiguousarray(ovov).reshape(ov, ov)
    Gx = np.ascontiguousarray(ovov.transpose(0, 3, 2, 1)).reshape(ov, ov)
    Gw = 2.0 * G - Gx
    H = np.ascontiguousarray(oovv.transpose(0, 2, 1, 3)).reshape(ov, ov)
    Moo = np.ascontiguousarray(oooo.transpose(0, 2, 1, 3)).reshape(o * o, o * o)
    Goo = np.ascontiguousarray(ovov.transpose(0, 2, 1, 3)).reshape(o * o, v * v)
    g = ovov.transpose(0, 2, 1, 3)
    # the two-electron part of the Fock matrix in the window's own orbitals, virtual block: sum_k 2 (kk|ac) - (ka|kc)
    G2e = 2.0 * np.einsum("kkac->ac", oovv) - np.einsum("kakc->ac", ovov)
    full, quad = method == "CCSD", method != "LCCSD"

    def step(t1, t2):
        th = t2 + np.einsum("ia,jb->ijab", t1, t1) if full else t2
        thf = np.ascontiguousarray(th).reshape(o * o, v, v)
        Bv = Cv @ t1.T                                                                       # b_i = C_v t_i, [N][o]
        Yvv, Zov = np.empty((o * o, v, v)), np.empty((o * o, o, v))
        counts["loops"] += 1
        for s0 in range(0, o * o, batch):
            T = np.matmul(Cv, np.matmul(thf[s0:s0 + batch], Cv.T))
            for n in range(T.shape[0]):
                i, j = divmod(s0 + n, o)
                T[n] += np.outer(Co[:, i], Bv[:, j]) + np.outer(Bv[:, i], Co[:, j])
            Z = np.asarray(Z_of(T)).reshape(T.shape)
            counts["Z_of"] += 1
            Yvv[s0:s0 + batch] = 0.5 * np.matmul(Cv.T, np.matmul(Z, Cv))
            Zov[s0:s0 + batch] = np.matmul(Co.T, np.matmul(Z, Cv))
        Zov = Zov.reshape(o, o, o, v)                                                        # [i j][k][a] = sum (k la|a si) T_ij
        t2f = np.ascontiguousarray(t2).reshape(o * o, v * v)
        thm = thf.reshape(o * o, v * v)
        Tn = np.ascontiguousarray(t2.transpose(0, 2, 1, 3)).reshape(ov, ov)
        Tx = np.ascontiguousarray(t2.transpose(0, 3, 1, 2)).reshape(ov, ov)
        # ---- singles: the ov blocks hold the th part, sum_kc [2 (ia|kc) - (ik|ac)] t_kc, and sum_c G2e_ca t_ic on top
        s = 2.0 * np.einsum("kika->ia", Zov) - np.einsum("ikka->ia", Zov) - t1 @ G2e
        s += -2.0 * np.einsum("iklc,klac->ia", ooov, th, optimize=True) + np.einsum("ilkc,klac->ia", ooov, th, optimize=True)
        A1, A2, W = G, H, Moo
        X = np.zeros((o * o, v * v))
        if quad:
            Tnh = np.ascontiguousarray(th.transpose(0, 2, 1, 3)).reshape(ov, ov) if full else Tn
            F_ik = Tnh.reshape(o, v * ov) @ Gw.reshape(o, v * ov).T
            F_ca = -sum(Gw.reshape(o, v, ov)[k_] @ Tnh.reshape(o, v, ov)[k_].T for k_ in range(o))
            F_kc = (Gw @ t1.ravel()).reshape(o, v)
            s += t1 @ F_ca - F_ik @ t1 + ((2.0 * Tn - Tx) @ F_kc.ravel()).reshape(o, v)
            W = Moo + thm @ Goo.T
            L_ca, L_ik = F_ca, F_ik
            if full:
                s += np.einsum("kc,ic,ka->ia", F_kc, t1, t1, optimize=True)
                P = np.einsum("jlkc,ic->ijkl", ooov, t1, optimize=True)
                W = W + (P + P.transpose(1, 0, 3, 2)).reshape(o * o, o * o)
                Lo, Xv = Co + Bv, Cv - Co @ t1
                A1 = np.ascontiguousarray(mo_of(Lo, Xv, Co, Cv)).reshape(ov, ov)             # (L_i X_a|kc)
                A2 = np.ascontiguousarray(np.asarray(mo_of(Lo, Co, Xv, Cv)).transpose(0, 2, 1, 3)).reshape(ov, ov)   # (L_i k|X_a c)
                counts["mo_of"] += 2
                J, K = jk_of(Co @ t1 @ Cv.T)
                counts["jk_of"] += 1
                M = 2.0 * np.asarray(J) - np.asarray(K)
                L_ca, L_ik = F_ca + Cv.T @ M @ Cv, F_ik + Co.T @ M @ Co
            A1 = A1 + 0.5 * (Tn @ Gw) - 0.5 * (Tx @ G)
            A2 = A2 - 0.5 * (Tx @ Gx)
            X = np.matmul(L_ca.T, t2f.reshape(o * o, v, v)).reshape(o * o, v * v) - (L_ik @ t2f.reshape(o, o * v * v)).reshape(o * o, v * v)
        X = X + 0.5 * (W @ thm)
        S1 = A1 @ (2.0 * Tn - Tx) - A2 @ Tn
        S2 = A2 @ Tx
        R = (0.5 * g + Yvv.reshape(o, o, v, v) + X.reshape(o, o, v, v) + S1.reshape(o, v, o, v).transpose(0, 2, 1, 3)
             - S2.reshape(o, v, o, v).transpose(0, 2, 3, 1))
        R = R - np.einsum("jkia,kb->ijab", ooov, t1, optimize=True)
        if full:
            R = R - np.einsum("ka,ijkb->ijab", t1, Zov, optimize=True)
        return s / D1, (R + R.transpose(1, 0, 3, 2)) / D2
    return _run(step, _energy_parts(ovov), g / D2, (o, v), method, k, **loop)
