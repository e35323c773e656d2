"""CPU: tests/triples_reference.py, the checker of the GPU triples tests, against the reference program's own results
(tests/golden/triples_systems.npz: the MP4 triples on every system from the golden orbitals and MO integrals of the oracle; CCSD(T) and
QCISD(T) on the two systems whose converged amplitudes the file holds) and against a dense six-index evaluation in the reference's own
arrangement -- the (4, 1, 1, -4, -1, -1) combination of permutations of (i, j, k) -- with non-symmetric random t2, where only the total
agrees; the symmetry of e_ijk and its diagonal."""
import itertools

import numpy as np
import pytest

import mp3_reference as mr
import triples_reference as tr
from test_ccd_reference import split
from test_gpu_mp3 import SYSTEMS
from tuna_amd import molecule as mol

TAGS = ["n2_ccpvdz", "n2_ccpvtz", "co_631g", "hf_ccpvdz", "ne_ccpvdz"]


@pytest.fixture(scope="module")
def triples_golden(golden):
    return split(golden("triples_systems"))


@pytest.fixture(scope="module")
def mp3_golden(golden):
    return split(golden("mp3_systems"))


def _blocks(tag, C, nocc, nf):
    sym, R, basis = SYSTEMS[tag]
    shells = mol.build_shells(mol.make_atoms(sym, R), basis)
    E = mr.dense_eri(mol.expand_cartesian_aos(shells), shells)
    Co, Cv = C[:, nf:nocc], C[:, nocc:]
    return mr.mo_tensor(E, Co, Cv, Co, Cv), mr.mo_tensor(E, Co, Cv, Cv, Cv), mr.mo_tensor(E, Co, Cv, Co, Co)


@pytest.mark.parametrize("tag", TAGS)
def test_checker_against_the_reference_program(triples_golden, mp3_golden, tag):
    g, m = triples_golden[tag], mp3_golden[tag]
    nocc, C, eps = int(m["n_occ"]), m["C"], m["eps"]
    for nf in (0, 1):
        blocks = _blocks(tag, C, nocc, nf)
        r = tr.triples(eps[nf:nocc], eps[nocc:], *blocks, "MP4")
        want = float(g[f"MP4_fc{nf}_E_T"])
        print(f"\n[{tag} fc{nf}] MP4 E_T {r['E_T']:.13f} golden {want:.13f} d {r['E_T'] - want:.1e}")
        assert abs(r["E_T"] - want) < 1e-11 and r["E_disconnected"] == 0.0
        if f"CCSD_fc{nf}_t2" not in g:
            continue
        for method in ("CCSD", "QCISD"):
            r = tr.triples(eps[nf:nocc], eps[nocc:], *blocks, f"{method}(T)", t1=g[f"{method}_fc{nf}_t1"], t2=g[f"{method}_fc{nf}_t2"])
            want = float(g[f"{method}_fc{nf}_E_T"])
            print(f"[{tag} fc{nf}] {method}(T) E_T {r['E_T']:.13f} golden {want:.13f} d {r['E_T'] - want:.1e}")
            assert abs(r["E_T"] - want) < 1e-11


def test_amplitudes_are_stored_for_two_systems(triples_golden):
    assert {t for t, g in triples_golden.items() if "CCSD_fc0_t2" in g} == {"co_631g", "ne_ccpvdz"}
    assert set(triples_golden) == set(TAGS)


def _dense(eo, ev, ovov, ovvv, ovoo, t1, t2, s):
    """E_T with dense o^3 v^3 arrays, in the reference's arrangement: W from the six column permutations, then 4 W + W_kij + W_jki
    - 4 W_kji - W_ikj - W_jik over the OCCUPIED indices"""
    X = np.einsum("iabf,kjcf->ijkabc", ovvv, t2) - np.einsum("iajm,mkbc->ijkabc", ovoo, t2)
    W = sum(X.transpose(*p, *(3 + q for q in p)) for p in itertools.permutations(range(3)))
    V = s * (np.einsum("jbkc,ia->ijkabc", ovov, t1) + np.einsum("iakc,jb->ijkabc", ovov, t1) + np.einsum("iajb,kc->ijkabc", ovov, t1))
    Wb = (4 * W + W.transpose(2, 0, 1, 3, 4, 5) + W.transpose(1, 2, 0, 3, 4, 5) - 4 * W.transpose(2, 1, 0, 3, 4, 5) - W.transpose(0, 2, 1, 3, 4, 5)
          - W.transpose(1, 0, 2, 3, 4, 5))
    n = None
    D = (eo[:, n, n, n, n, n] + eo[n, :, n, n, n, n] + eo[n, n, :, n, n, n] - ev[n, n, n, :, n, n] - ev[n, n, n, n, :, n] - ev[n, n, n, n, n, :])
    per_triple = ((W + V) * Wb / D).sum(axis=(3, 4, 5)) / 3.0
    return float(per_triple.sum()), per_triple


@pytest.mark.parametrize("o,v", [(3, 4), (2, 4), (1, 5), (3, 5), (3, 1), (2, 2)])
def test_checker_against_the_dense_six_index_form(o, v):
    rng = np.random.default_rng(10 * o + v)
    n = o + v
    g = rng.standard_normal((n,) * 4)
    g = g + g.transpose(1, 0, 2, 3)
    g = g + g.transpose(0, 1, 3, 2)
    g = g + g.transpose(2, 3, 0, 1)                                   # 8-fold symmetric "integrals"
    eps = np.sort(rng.standard_normal(n))
    eps[:o] -= 2.0
    ovov, ovvv, ovoo = tr.blocks_from_g(g, 0, o)
    eo, ev = eps[:o], eps[o:]
    t1, t2 = rng.standard_normal((o, v)), rng.standard_normal((o, o, v, v))          # t2 NOT symmetric under (ij)(ab)
    for kind, s in (("CCSD(T)", 1.0), ("QCISD(T)", 2.0)):
        r = tr.triples(eo, ev, ovov, ovvv, ovoo, kind, t1=t1, t2=t2)
        want, per_triple = _dense(eo, ev, ovov, ovvv, ovoo, t1, t2, s)
        N = float(r["N_ijk"].sum())
        print(f"\n[o {o} v {v} {kind}] E_T {r['E_T']:.12e} dense {want:.12e} |d|/N {abs(r['E_T'] - want) / N:.1e}")
        assert abs(r["E_T"] - want) <= 1e-14 * N
        assert abs(r["E_T"] - (r["E_connected"] + r["E_disconnected"])) <= 1e-14 * N
        # symmetric under every permutation of (i, j, k), exactly (computed once and scattered); the diagonal is rounding noise
        for p in itertools.permutations(range(3)):
            assert np.array_equal(r["e_ijk"], r["e_ijk"].transpose(p)) and np.array_equal(r["S_ijk"], r["S_ijk"].transpose(p))
        diag = np.abs(np.einsum("iii->i", r["e_ijk"]))
        assert np.all(diag <= 1e-15 * np.einsum("iii->i", r["N_ijk"])), diag
        if o >= 2 and v >= 2:                                         # (with o = 1 or v = 1 every bracket cancels: S itself is noise, N is the scale)
            assert np.all(diag <= 1e-15 * r["S_ijk"].sum()), diag
        # the reference's per-triple terms are not symmetric; their average over the six orderings is e_ijk
        avg = sum(per_triple.transpose(p) for p in itertools.permutations(range(3))) / 6.0
        assert np.abs(avg - r["e_ijk"]).max() <= 1e-14 * r["N_ijk"].max()
    # MP4: first-order amplitudes, V = 0
    r = tr.triples(eo, ev, ovov, ovvv, ovoo, "MP4")
    want, _ = _dense(eo, ev, ovov, ovvv, ovoo, np.zeros((o, v)), tr.mp2_amplitudes(ovov, eo, ev), 0.0)
    assert abs(r["E_T"] - want) <= 1e-14 * float(r["N_ijk"].sum()) and r["E_disconnected"] == 0.0
    # only = a subset: the rest stays out
    if o >= 2:
        part = tr.triples(eo, ev, ovov, ovvv, ovoo, "MP4", only=[(1, 0, 0)])
        assert np.isnan(part["e_ijk"][0, 0, 0]) and part["e_ijk"][0, 1, 0] == r["e_ijk"][1, 0, 0] and abs(part["E_T"] - 3 * r["e_ijk"][1, 0, 0]) < 1e-13 * abs(want) + 1e-300
