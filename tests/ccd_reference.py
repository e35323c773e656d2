"""Independent NumPy LCCD / CCD for the tests: the doubles amplitude iteration from canonical RHF orbitals (occupied window
[n_frozen, n_occ), virtual window [n_occ, N)), D = e_i + e_j - e_a - e_b, guess t_ijab = (ia|jb) / D, E = sum [2 (ia|jb) - (ib|ja)] t_ijab,
in three forms:
  * restricted_iterations: the closed-shell equations in chemists' notation on dense MO blocks of a dense spherical (mu nu|la si)
    tensor, (ac|bd) included;
  * spin_orbital_iterations: the textbook spin-orbital doubles equations (Shavitt and Bartlett, Many-Body Methods in Chemistry and
    Physics, eq. 9.126; LCCD keeps the terms linear in t) on the antisymmetrised <pq||rs> of the spin orbitals (p alpha, p beta) of the
    same spatial orbitals; its alpha-beta block t[i alpha, j beta, a alpha, b beta] is the closed-shell t_ijab;
  * iterations_from_blocks: the restricted equations from the three blocks (ia|jb), (ij|ab), (ik|jl) and a callback Z_of that maps AO
    matrices T to Z[T][mu][nu] = sum (mu la|nu si) T[la][si]; never forms (ac|bd); explicit reshaped GEMMs.
All three run the same loop (iterate): new amplitudes; energy and dE (the first dE from zero); converged if |dE| < conv_delta_E and
||t - t_old||_2 < amp_conv; otherwise (t, t - t_old) join the DIIS history, from step 3 on the oldest pair beyond max_diis leaves and the
amplitudes are extrapolated (B matrix with -1 borders; a singular B clears the history), then t <- damping t_old + (1 - damping) t.
Each returns {"t", "energies", "n_iter", "converged", "E_MP2"}; t and E are those of the last step taken."""
from __future__ import annotations

import numpy as np

from mp3_reference import _so_block, _windows, mo_tensor


def iterate(step, energy, t0, k, conv_delta_E=0.0, amp_conv=0.0, diis=False, max_diis=6, damping=0.0, norm=None):
    """k steps at most of t <- step(t); norm(dt) defaults to the 2-norm of all elements."""
    norm = norm or (lambda d: float(np.linalg.norm(d)))
    t, E, energies, hist_t, hist_e, converged = t0, 0.0, [], [], [], False
    new = t0
    for n in range(1, k + 1):
        E_old, old = E, t
        new = step(old)
        E = float(energy(new))
        energies.append(E)
        if abs(E - E_old) < conv_delta_E and norm(new - old) < amp_conv:
            converged = True
            break
        if n == k:
            break
        t = new
        if diis:
            hist_t.append(new.copy())
            hist_e.append((new - old).ravel())
            if n > 2:
                if len(hist_e) > max_diis:
                    del hist_t[0], hist_e[0]
                m = len(hist_e)
                B = -np.ones((m + 1, m + 1))
                B[m, m] = 0.0
                for p in range(m):
                    for q in range(m):
                        B[p, q] = float(hist_e[p] @ hist_e[q])
                rhs = np.zeros(m + 1)
                rhs[m] = -1.0
                try:
                    c = np.linalg.solve(B, rhs)[:m]
                    t = sum(c[p] * hist_t[p] for p in range(m))
                except np.linalg.LinAlgError:
                    hist_t.clear()
                    hist_e.clear()
        t = damping * old + (1.0 - damping) * t
    return {"t": new, "energies": energies, "n_iter": len(energies), "converged": converged}


def _denominators(eo, ev):
    return eo[:, None, None, None] + eo[None, :, None, None] - ev[None, None, :, None] - ev[None, None, None, :]


def _restricted_energy(ovov):
    w = (2.0 * ovov - ovov.transpose(0, 3, 2, 1)).transpose(0, 2, 1, 3)       # [i j a b]: 2 (ia|jb) - (ib|ja)
    return lambda t: np.sum(w * t)


def restricted_step(ovov, oovv, oooo, ladder, D, method):
    """t -> t_new.  ovov[i a j b] = (ia|jb), oovv[i j a b] = (ij|ab), oooo[i k j l] = (ik|jl); ladder(t)[i j a b] = 1/2 sum_cd (ac|bd) t_ijcd."""
    g = ovov.transpose(0, 2, 1, 3)                                            # [i j a b] = (ia|jb)

    def step(t):
        W_oooo = oooo.transpose(0, 2, 1, 3)                                   # [i j k l] = (ik|jl)
        W_icak = ovov                                                         # [i a k c] = (ia|kc)
        W_ciak = oovv.transpose(0, 2, 1, 3)                                   # [i a k c] = (ik|ac)
        R = 0.5 * g + ladder(t)
        if method == "CCD":
            w = 2.0 * ovov - ovov.transpose(0, 3, 2, 1)                       # [k c l d] = 2 (kc|ld) - (kd|lc)
            F_ik = np.einsum("kcld,ilcd->ik", w, t, optimize=True)
            F_ca = -np.einsum("kcld,klad->ca", w, t, optimize=True)
            W_oooo = W_oooo + np.einsum("kcld,ijcd->ijkl", ovov, t, optimize=True)
            W_icak = (ovov - 0.5 * np.einsum("ldkc,ilda->iakc", ovov, t, optimize=True)
                      + 0.5 * np.einsum("ldkc,ilad->iakc", w, t, optimize=True))
            W_ciak = W_ciak - 0.5 * np.einsum("lckd,ilda->iakc", ovov, t, optimize=True)
            R = R + np.einsum("ca,ijcb->ijab", F_ca, t, optimize=True) - np.einsum("ik,kjab->ijab", F_ik, t, optimize=True)
        elif method != "LCCD":
            raise ValueError(method)
        R = R + 0.5 * np.einsum("ijkl,klab->ijab", W_oooo, t, optimize=True)
        R = R + np.einsum("iakc,kjcb->ijab", 2.0 * W_icak - W_ciak, t, optimize=True)
        R = R - np.einsum("iakc,kjbc->ijab", W_icak, t, optimize=True)
        R = R - np.einsum("ibkc,kjac->ijab", W_ciak, t, optimize=True)
        return (R + R.transpose(1, 0, 3, 2)) / D
    return step


def restricted_iterations(E, C, eps, n_occ, n_frozen, method, k, **loop):
    Co, Cv, eo, ev = _windows(C, eps, n_occ, n_frozen)
    ovov, oovv = mo_tensor(E, Co, Cv, Co, Cv), mo_tensor(E, Co, Co, Cv, Cv)
    oooo, vvvv = mo_tensor(E, Co, Co, Co, Co), mo_tensor(E, Cv, Cv, Cv, Cv)
    D = _denominators(eo, ev)
    t0 = ovov.transpose(0, 2, 1, 3) / D
    energy = _restricted_energy(ovov)
    step = restricted_step(ovov, oovv, oooo, lambda t: 0.5 * np.einsum("acbd,ijcd->ijab", vvvv, t, optimize=True), D, method)
    return dict(iterate(step, energy, t0, k, **loop), E_MP2=float(energy(t0)))


def spin_orbital_iterations(E, C, eps, n_occ, n_frozen, method, k, **loop):
    """The alpha-beta block of the spin-orbital amplitudes comes back as "t" ([i j a b], spatial indices), the full array as "t_so".
    The amplitude norm of the convergence test is taken over the alpha-beta block, as the restricted iteration takes it."""
    C, eps = np.asarray(C, float), np.asarray(eps, float)
    N = C.shape[0]
    g = mo_tensor(E, C, C, C, C)
    occ, vir = np.arange(n_frozen, n_occ), np.arange(n_occ, N)
    D = _denominators(np.repeat(eps[occ], 2), np.repeat(eps[vir], 2))
    oovv, oooo = _so_block(g, occ, occ, vir, vir), _so_block(g, occ, occ, occ, occ)
    vvvv, ovvo = _so_block(g, vir, vir, vir, vir), _so_block(g, occ, vir, vir, occ)

    def P(X, ax1, ax2):
        return X - X.swapaxes(ax1, ax2)

    def step(t):
        R = oovv + 0.5 * np.einsum("abcd,ijcd->ijab", vvvv, t, optimize=True) + 0.5 * np.einsum("klij,klab->ijab", oooo, t, optimize=True)
        R = R + P(P(np.einsum("kbcj,ikac->ijab", ovvo, t, optimize=True), 0, 1), 2, 3)
        if method == "CCD":
            R = R + 0.25 * np.einsum("klcd,ijcd,klab->ijab", oovv, t, t, optimize=True)
            R = R + P(np.einsum("klcd,ikac,jlbd->ijab", oovv, t, t, optimize=True), 0, 1)
            R = R - 0.5 * P(np.einsum("klcd,ikdc,ljab->ijab", oovv, t, t, optimize=True), 0, 1)
            R = R - 0.5 * P(np.einsum("klcd,lkac,ijdb->ijab", oovv, t, t, optimize=True), 2, 3)
        elif method != "LCCD":
            raise ValueError(method)
        return R / D

    def ab(t):
        return t[0::2, 1::2, 0::2, 1::2]
    r = iterate(step, lambda t: 0.25 * np.sum(oovv * t), oovv / D, k, norm=lambda d: float(np.linalg.norm(ab(d))), **loop)
    return dict(r, t=np.ascontiguousarray(ab(r["t"])), t_so=r["t"], E_MP2=float(0.25 * np.sum(oovv * oovv / D)))


def iterations_from_blocks(ovov, oovv, oooo, Z_of, Cv, eo, ev, method, k, batch=64, **loop):
    """ovov[i a j b] = (ia|jb), oovv[i j a b] = (ij|ab), oooo[i k j l] = (ik|jl).  Matrices over (ov) x (ov) unless noted:
    G[(ia)][(kc)] = (ia|kc), Gx[(ld)][(kc)] = (lc|kd), H[(ia)][(kc)] = (ik|ac), Tn[(kc)][(jb)] = t_kjcb, Tx[(kc)][(jb)] = t_kjbc."""
    o, v = len(eo), len(ev)
    ov = o * v
    D = _denominators(eo, ev)
    G = np.ascontiguousarray(ovov).reshape(ov, ov)
    Gx = np.ascontiguousarray(ovov.transpose(0, 3, 2, 1)).reshape(ov, ov)
    Gw = 2.0 * G - Gx
    H = np.ascontiguousarray(oovv.transpose(0, 2, 1, 3)).reshape(ov, ov)
    Moo = np.ascontiguousarray(oooo.transpose(0, 2, 1, 3)).reshape(o * o, o * o)             # [(ij)][(kl)] = (ik|jl)
    Goo = np.ascontiguousarray(ovov.transpose(0, 2, 1, 3)).reshape(o * o, v * v)             # [(kl)][(cd)] = (kc|ld)
    g = ovov.transpose(0, 2, 1, 3)

    def step(t):
        tf = np.ascontiguousarray(t).reshape(o * o, v, v)
        X_pp = np.empty((o * o, v, v))
        for s in range(0, o * o, batch):
            T = np.matmul(Cv, np.matmul(tf[s:s + batch], Cv.T))
            Z = np.asarray(Z_of(T)).reshape(T.shape)
            X_pp[s:s + batch] = 0.5 * np.matmul(Cv.T, np.matmul(Z, Cv))
        Tn = np.ascontiguousarray(t.transpose(0, 2, 1, 3)).reshape(ov, ov)
        Tx = np.ascontiguousarray(t.transpose(0, 3, 1, 2)).reshape(ov, ov)
        t2 = tf.reshape(o * o, v * v)
        A1, A2, W = G, H, Moo
        X = np.zeros((o * o, v * v))
        if method == "CCD":
            F_ik = Tn.reshape(o, v * ov) @ Gw.reshape(o, v * ov).T
            F_ca = -sum(Gw.reshape(o, v, ov)[k_] @ Tn.reshape(o, v, ov)[k_].T for k_ in range(o))
            W = Moo + t2 @ Goo.T
            A1 = G + 0.5 * (Tn @ Gw) - 0.5 * (Tx @ G)
            A2 = H - 0.5 * (Tx @ Gx)
            X = np.matmul(F_ca.T, tf).reshape(o * o, v * v) - (F_ik @ t2.reshape(o, o * v * v)).reshape(o * o, v * v)
        elif method != "LCCD":
            raise ValueError(method)
        X = X + 0.5 * (W @ t2)
        S1 = A1 @ (2.0 * Tn - Tx) - A2 @ Tn                                                  # [(ia)][(jb)]
        S2 = A2 @ Tx                                                                         # [(ib)][(ja)]
        R = (0.5 * g + X_pp.reshape(o, o, v, v) + X.reshape(o, o, v, v) + S1.reshape(o, v, o, v).transpose(0, 2, 1, 3)
             - S2.reshape(o, v, o, v).transpose(0, 2, 3, 1))
        return (R + R.transpose(1, 0, 3, 2)) / D
    energy = _restricted_energy(ovov)
    t0 = g / D
    return dict(iterate(step, energy, t0, k, **loop), E_MP2=float(energy(t0)))
