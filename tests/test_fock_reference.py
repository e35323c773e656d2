"""CPU: tests/fock_reference.py -- the shape table sits on the edges it names (widths computed from the shell lists through
layout_model.Layout), and the references agree with two independent restatements: the NumPy model of the packed algorithm
(layout_model.fock_partial) and the oracle's own contractions (so.coulomb / so.exchange: "ijkl,kl->ij", "ilkj,kl->ij") on the oracle
tensor of every shape."""
import numpy as np
import pytest

import fock_reference as fr
import layout_model as lm
from oracle import scf_oracle as so
from ump2_reference import dense_eri

_TENSORS = {}


def oracle_tensor(tag):
    if tag not in _TENSORS:
        _, shells, aos = fr.system(tag)
        _TENSORS[tag] = dense_eri(aos, shells)
    return _TENSORS[tag]


@pytest.mark.parametrize("tag", list(fr.SHAPES))
def test_shape_table_sits_on_its_edges(tag):
    _, shells, aos = fr.system(tag)
    _, _, N, widths = fr.SHAPES[tag]
    L = fr.layout_of(shells)
    assert L.N == N == sum(s.n_sph for s in shells) and tuple(int(x) for x in L.csize) == widths
    assert max(float(s.exps.max()) for s in shells) < 3.0 and all(len(s.exps) == 1 for s in shells)
    if tag in fr.CARTESIAN_TAGS:
        Lc = fr.layout_of(shells, spherical=False)
        assert Lc.N == aos.n == sum(s.n_cart for s in shells)


def test_the_edges_are_all_in_the_table():
    """every shape constant has a width below it, on it and above it (or the widths the issue names for it)"""
    c0 = {w[0] for _, _, _, w in fr.SHAPES.values()}
    for edge in (8, 16, 32, 64):
        assert {edge - 1, edge, edge + 1} <= c0, edge
    rest = {w[1:] for _, _, _, w in fr.SHAPES.values()}
    assert (16, 16, 8) in rest and (17, 17, 9) in rest and (0, 0, 0) in rest and (1, 1, 0) in rest and (3, 3, 0) in rest


@pytest.mark.parametrize("tag", ["c0_65", "mid_17_9", "sp", "one_s"])
def test_edge_aos(tag):
    L = fr.layout_of(fr.system(tag)[1])
    aos = fr.edge_aos(L)
    assert aos == sorted(set(aos)) == fr.edge_aos(L) and len(aos) <= 30 and all(0 <= a < L.N for a in aos)
    locs = {(int(L.cls[a]), int(L.loc[a])) for a in aos}
    for c in range(4):
        n = int(L.csize[c])
        for lam in (0, n - 1) + fr.LOC_EDGES:
            assert n == 0 or lam >= n or (c, lam) in locs, (c, lam)
    pairs = fr.probe_pairs(L)
    assert all(k >= l for k, l in pairs) and len(pairs) == len(set(pairs))
    if L.N <= 20:
        assert len(pairs) == L.N * (L.N + 1) // 2
    else:
        assert len(pairs) == len(aos) * (len(aos) + 1) // 2 <= 465


@pytest.mark.parametrize("tag", ["one_d", "c0_9"])
def test_references_against_the_model_of_the_packed_algorithm(tag):
    """layout_model.fock_partial (the kernel's task structure, its halved diagonal terms and its reductions, in float64) on the oracle
    tensor: random densities within the bound of fock_reference.random_bound; every unit density J exactly, K within 4 roundings of S"""
    E = fr.canonical_copy(oracle_tensor(tag))                             # (the model reads the stored image of an element only)
    L = fr.layout_of(fr.system(tag)[1])
    N = L.N
    assert np.array_equal(E, E.transpose(1, 0, 2, 3)) and np.array_equal(E, E.transpose(2, 3, 0, 1)) and np.abs(E - oracle_tensor(tag)).max() < 1e-15
    rows = [(i, j) for i in range(N) for j in range(i + 1)]
    S, _ = fr.random_densities(N, 2)
    J, K, AJ, AK = fr.reference_jk(E, S)
    for d in range(2):
        Jm, Km, _ = lm.fock_partial(L, E, S[d], rows)
        assert np.all(np.abs(Jm - J[d]) <= fr.random_bound(N) * AJ[d]) and np.all(np.abs(Km - K[d]) <= fr.random_bound(N) * AK[d])
    forbidden = ~fr.allowed_mask(L.cls)
    worst = 0.0
    pairs = fr.probe_pairs(L)
    Jw, Kw, Sw = fr.unit_expectations(E, pairs)
    for n, (k, l) in enumerate(pairs):
        Jm, Km, _ = lm.fock_partial(L, E, fr.unit_density(N, k, l), rows)
        J1, K1, S1 = fr.unit_expectation(E, k, l)
        assert np.array_equal(J1, Jw[n]) and np.array_equal(K1, Kw[n]) and np.array_equal(S1, Sw[n])
        assert np.array_equal(Jm, J1), (k, l)
        assert np.all(np.abs(Km - K1) <= 4 * fr.EPS * S1), (k, l)
        assert np.all(Jm[forbidden[:, :, k, l]] == 0.0) and np.all(Km[forbidden[:, :, k, l]] == 0.0)
        worst = max(worst, float(np.max(np.abs(Km - K1) / np.where(S1 > 0, fr.EPS * S1, 1.0))))
    print(f"\n[{tag}] {len(pairs)} unit probes through the model: worst K ratio {worst:.2f} (bound 4)")


@pytest.mark.parametrize("tag", list(fr.SHAPES))
def test_references_against_the_oracle_contractions(tag):
    """so.coulomb / so.exchange (float64 einsum) on the oracle tensor: a different order of the same sum, inside the derived bound"""
    E = oracle_tensor(tag)
    L = fr.layout_of(fr.system(tag)[1])
    N = L.N
    assert E.shape == (N,) * 4 and np.all(E[~fr.allowed_mask(L.cls)] == 0.0)
    S, G = fr.random_densities(N, 2)
    P = np.concatenate([S, G[None]])
    R = fr.Reference(E)                                                    # (what reference_jk makes per call)
    J, K, AJ, AK = R.jk(P)
    assert J.dtype == np.longdouble and K.dtype == np.longdouble and J.shape == P.shape
    worst = 0.0
    for d in range(3):
        Jo, Ko = so.coulomb(P[d], E), so.exchange(P[d], E)
        assert np.all(np.abs(Jo - J[d]) <= fr.random_bound(N) * AJ[d]) and np.all(np.abs(Ko - K[d]) <= fr.random_bound(N) * AK[d])
        worst = max(worst, float(np.max(np.abs(Jo - J[d]) / (fr.EPS * AJ[d]))), float(np.max(np.abs(Ko - K[d]) / (fr.EPS * AK[d]))))
    J1, K1, AJ1, AK1 = fr.reference_jk(E, G)                               # one [N,N] density: the same numbers
    assert np.array_equal(J1, J[2]) and np.array_equal(K1, K[2])
    assert np.allclose(AJ1, AJ[2], rtol=1e-13, atol=0) and np.allclose(AK1, AK[2], rtol=1e-13, atol=0)  # (float64 BLAS: the order may differ)
    pairs = fr.probe_pairs(L)
    for k, l in pairs[::max(1, len(pairs) // 3)]:
        Pu = fr.unit_density(N, k, l)
        Jw, Kw, Sw = fr.unit_expectation(E, k, l)
        skew = np.abs(E[:, :, k, l] - E[:, :, l, k])                       # (the oracle's dense tensor is 8-fold symmetric to rounding only)
        assert np.all(np.abs(so.coulomb(Pu, E) - Jw) <= 2 * fr.EPS * np.abs(Jw) + skew), (k, l)
        assert np.all(np.abs(so.exchange(Pu, E) - Kw) <= 4 * fr.EPS * Sw), (k, l)
        Jl, Kl, _, AKl = R.jk(Pu)
        assert np.all(np.abs(Jl - Jw) <= skew) and np.all(np.abs(Kl - Kw) <= fr.EPS * Sw) and np.all(AKl <= Sw * (1 + 2 * fr.EPS))
    print(f"\n[{tag}] N = {N}: float64 einsum against the longdouble reference, worst ratio {worst:.2f} (bound {N * N + 4})")
