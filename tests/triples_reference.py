"""Independent NumPy (T): the perturbative triples of CCSD(T), QCISD(T) and full MP4 for a closed shell, one unordered triple of occupied
orbitals and one v^3 array at a time.  Chemists' integrals; ovov[i,a,j,b] = (ia|jb), ovvv[i,a,b,f] = (ia|bf), ovoo[i,a,j,m] = (ia|jm):

    X_ijk^abc = sum_f (ia|bf) t2[k,j,c,f] - sum_m (ia|jm) t2[m,k,b,c]
    W_ijk^abc = the sum over the six simultaneous permutations of the columns (i a), (j b), (k c) of X
    V_ijk^abc = s [(jb|kc) t1[i,a] + (ia|kc) t1[j,b] + (ia|jb) t1[k,c]]            s = 1 (CCSD(T)), 2 (QCISD(T)), V = 0 (MP4)
    D_ijk^abc = e_i + e_j + e_k - e_a - e_b - e_c
    e_ijk     = 1/3 sum_abc (W + V)^abc (4 W^abc + W^bca + W^cab - 2 W^cba - 2 W^acb - 2 W^bac) / D
    E_T       = the sum of e_ijk over all ordered (i, j, k)

e_ijk is symmetric in (i, j, k): every unordered triple i >= j >= k is computed once (the diagonal i = j = k too: it comes out as
rounding noise around 0) and scattered.  S_ijk = 1/3 sum_abc |(W + V) (...) / D| is the sum of the magnitudes that e_ijk adds up: the
scale of its rounding error.  Where the bracket cancels term by term (i = j = k; o = 1; v = 1) S itself is rounding noise; N_ijk, the same
sum with every W, V and D replaced by its magnitude, is the scale there."""
import itertools

import numpy as np

PERMS = list(itertools.permutations(range(3)))
SCALE = {"CCSD(T)": 1.0, "QCISD(T)": 2.0, "MP4": 0.0}


def _x(ovvv, ovoo, t2, p, q, r):
    """X_pqr[a, b, c] (two BLAS products)"""
    return ovvv[p] @ t2[r, q].T - np.tensordot(ovoo[p, :, q, :], t2[:, r], axes=(1, 0))


def _perm(A, s):
    """out[v0, v1, v2] = A[v_s0, v_s1, v_s2]"""
    return np.einsum(A, list(s), [0, 1, 2])


def mp2_amplitudes(ovov, eo, ev):
    D = eo[:, None, None, None] + eo[None, :, None, None] - ev[None, None, :, None] - ev[None, None, None, :]
    return ovov.transpose(0, 2, 1, 3) / D


def triples(eo, ev, ovov, ovvv, ovoo, kind="CCSD(T)", t1=None, t2=None, only=None):
    """{"E_T", "E_connected", "E_disconnected", "e_ijk", "c_ijk", "d_ijk" (the two parts of e_ijk), "S_ijk", "N_ijk"}; kind "MP4": t2 = (ia|jb) / D,
    V = 0.  only = an iterable of unordered triples (i >= j >= k): the others stay NaN in the arrays and out of the sums."""
    o, v = len(eo), len(ev)
    s = SCALE[kind]
    if kind == "MP4":
        assert t1 is None and t2 is None
        t2 = mp2_amplitudes(ovov, eo, ev)
    c_ijk, d_ijk, S_ijk, N_ijk = (np.full((o, o, o), np.nan) for _ in range(4))
    todo = [(i, j, k) for i in range(o) for j in range(i + 1) for k in range(j + 1)] if only is None else [tuple(t) for t in only]
    Dv = -(ev[:, None, None] + ev[None, :, None] + ev[None, None, :])
    for i, j, k in todo:
        occ = (i, j, k)
        W = np.zeros((v, v, v))
        for sg in PERMS:
            W += _perm(_x(ovvv, ovoo, t2, occ[sg[0]], occ[sg[1]], occ[sg[2]]), sg)
        Y = 4.0 * W + _perm(W, (1, 2, 0)) + _perm(W, (2, 0, 1)) - 2.0 * _perm(W, (2, 1, 0)) - 2.0 * _perm(W, (0, 2, 1)) - 2.0 * _perm(W, (1, 0, 2))
        Y /= eo[i] + eo[j] + eo[k] + Dv
        A = np.abs(W)
        Ya = (4.0 * A + _perm(A, (1, 2, 0)) + _perm(A, (2, 0, 1)) + 2.0 * _perm(A, (2, 1, 0)) + 2.0 * _perm(A, (0, 2, 1)) + 2.0 * _perm(A, (1, 0, 2))) / \
            np.abs(eo[i] + eo[j] + eo[k] + Dv)
        V = 0.0 * W
        if s != 0.0:
            V = s * (np.einsum("bc,a->abc", ovov[j, :, k, :], t1[i]) + np.einsum("ac,b->abc", ovov[i, :, k, :], t1[j]) +
                     np.einsum("ab,c->abc", ovov[i, :, j, :], t1[k]))
        c, d, S = (W * Y).sum() / 3.0, (V * Y).sum() / 3.0, np.abs((W + V) * Y).sum() / 3.0
        Nn = ((A + np.abs(V)) * Ya).sum() / 3.0
        for p in set(itertools.permutations(occ)):
            c_ijk[p], d_ijk[p], S_ijk[p], N_ijk[p] = c, d, S, Nn
    e_ijk = c_ijk + d_ijk
    return {"E_T": float(np.nansum(e_ijk)), "E_connected": float(np.nansum(c_ijk)), "E_disconnected": float(np.nansum(d_ijk)), "e_ijk": e_ijk,
            "c_ijk": c_ijk, "d_ijk": d_ijk, "S_ijk": S_ijk, "N_ijk": N_ijk}


def blocks_from_g(g, nf, nocc):
    """(eo-independent) ovov, ovvv, ovoo from a full chemists' MO tensor g[p,q,r,s] = (pq|rs)"""
    o, v = slice(nf, nocc), slice(nocc, g.shape[0])
    return g[o, v, o, v], g[o, v, v, v], g[o, v, o, o]
