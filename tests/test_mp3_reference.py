"""CPU: the independent MP3 of tests/mp3_reference.py against the reference program's own run_restricted_MP3
(tests/golden/mp3_systems.npz, tools/make_golden_mp3.py) on the golden orbitals, frozen-core variants included; and the AO-direct
particle-particle ladder (the route of the library) against the MO-basis ladder on random data.  tests/test_gpu_mp3.py then judges the
library by it."""
import numpy as np
import pytest

import mp3_reference as mr
from conftest import R_N2
from tuna_amd import molecule as mol

SYSTEMS = {"n2_sto3g": (["N", "N"], R_N2, "STO-3G"), "n2_ccpvdz": (["N", "N"], R_N2, "cc-pVDZ"), "n2_ccpvtz": (["N", "N"], R_N2, "cc-pVTZ"),
           "co_631g": (["C", "O"], mol.angstrom_to_bohr(1.128), "6-31G"), "hf_ccpvdz": (["F", "H"], mol.angstrom_to_bohr(0.917), "cc-pVDZ"),
           "ne_ccpvdz": (["NE"], None, "cc-pVDZ")}


@pytest.fixture(scope="module")
def mp3_golden(golden):
    z = golden("mp3_systems")
    out = {}
    for key in z.files:
        tag, name = key.split("__", 1)
        out.setdefault(tag, {})[name] = z[key]
    return out


def dense(tag):
    sym, R, basis = SYSTEMS[tag]
    atoms = mol.make_atoms(sym, R)
    shells = mol.build_shells(atoms, basis)
    return mr.dense_eri(mol.expand_cartesian_aos(shells), shells)


@pytest.mark.parametrize("tag", list(SYSTEMS))
def test_spin_orbital_form_matches_reference_goldens(mp3_golden, tag):
    g = mp3_golden[tag]
    E = dense(tag)
    nocc = int(g["n_occ"])
    for nf, pre in ((0, ""), (1, "fc1_"), (2, "fc2_")):
        so = mr.spin_orbital_terms(E, g["C"], g["eps"], nocc, nf)
        assert abs(sum(so) - float(g[pre + "E_MP3"])) < 1e-10, (tag, nf, so, float(g[pre + "E_MP3"]))
        if tag != "n2_ccpvtz":                                      # (the dense v^4 block of the MO form: the smaller systems)
            rt = mr.restricted_terms(E, g["C"], g["eps"], nocc, nf)
            assert np.allclose(rt, so, rtol=0, atol=1e-11), (tag, nf, rt, so)


def test_scs_goldens_are_the_scaled_parts(mp3_golden):
    for tag, g in mp3_golden.items():
        want = float(g["E_SS"]) / 3 + 1.2 * float(g["E_OS"]) + 0.25 * float(g["E_MP3"])
        assert abs(float(g["scs_E_corr"]) - want) < 1e-12, tag


def _random_case(N, n_occ, seed):
    """A random 8-fold-symmetric tensor, random orthonormal orbitals, ascending eigenvalues with a gap at n_occ."""
    rng = np.random.default_rng(seed)
    E = rng.standard_normal((N, N, N, N))
    E = E + E.transpose(1, 0, 2, 3)
    E = E + E.transpose(0, 1, 3, 2)
    E = E + E.transpose(2, 3, 0, 1)
    C = np.linalg.qr(rng.standard_normal((N, N)))[0]
    eps = np.concatenate([-np.linspace(3.0, 0.5, n_occ), np.linspace(0.4, 4.0, N - n_occ)])
    return E, C, eps


@pytest.mark.parametrize("N, n_occ, n_frozen", [(9, 3, 0), (12, 5, 1), (14, 6, 2)])
def test_ao_direct_ladder_equals_mo_ladder(N, n_occ, n_frozen):
    E, C, eps = _random_case(N, n_occ, 100 + N)
    X, Z = mr.ao_direct_ladder(E, C, eps, n_occ, n_frozen)
    assert np.allclose(X, mr.mo_ladder(E, C, eps, n_occ, n_frozen), rtol=0, atol=1e-10 * np.abs(X).max())
    assert np.allclose(Z.transpose(1, 0, 3, 2), Z, rtol=0, atol=1e-12 * np.abs(Z).max())       # Z_ji = Z_ij^T
    # the stored-triangle identity the packed kernel uses: Z_ij = Zh_ij + Zh_ji^T, Zh from the pairs (nu si) <= (mu la), the diagonal halved
    Co, Cv = C[:, n_frozen:n_occ], C[:, n_occ:]
    t, _ = mr.amplitudes(mr.mo_tensor(E, Co, Cv, Co, Cv), eps[n_frozen:n_occ], eps[n_occ:])
    T = np.einsum("la,ijab,sb->ijls", Cv, t, Cv)
    hi, lo = np.maximum.outer(np.arange(N), np.arange(N)), np.minimum.outer(np.arange(N), np.arange(N))
    pid = hi * (hi + 1) // 2 + lo                                   # pair index of (a, b)
    keep = (pid[None, None, :, :] < pid[:, :, None, None]) + 0.5 * (pid[None, None, :, :] == pid[:, :, None, None])
    Lt = E * keep                                                   # L[(mu la)][(nu si)]
    Zh = np.einsum("mlns,ijls->ijmn", Lt, T)
    assert np.allclose(Zh + Zh.transpose(1, 0, 3, 2), Z, rtol=0, atol=1e-12 * np.abs(Z).max())


def test_spin_orbital_and_restricted_terms_agree_on_random_data():
    E, C, eps = _random_case(10, 4, 7)
    for nf in (0, 1):
        so, rt = mr.spin_orbital_terms(E, C, eps, 4, nf), mr.restricted_terms(E, C, eps, 4, nf)
        assert np.allclose(so, rt, rtol=1e-12, atol=1e-12 * max(abs(x) for x in so)), (nf, so, rt)


def _blocks_and_terms(E, C, eps, n_occ, n_frozen):
    """terms_from_blocks with every input made the way tests/test_gpu_mp3_large.py makes it: (ij|ab) and (ki|lj) from Coulomb matrices,
    Z from the exchange matrix of the transposed argument (the reference strings "ijkl,kl->ij" and "ilkj,kl->ij")."""
    Co, Cv, eo, ev = mr._windows(C, eps, n_occ, n_frozen)
    ovov = mr.mo_tensor(E, Co, Cv, Co, Cv)
    oovv, oooo = mr.blocks_from_coulomb(lambda D: np.einsum("ijkl,pkl->pij", E, D, optimize=True), Co, Cv, batch=5)
    return mr.terms_from_blocks(ovov, oovv, oooo, lambda T: np.einsum("ilkj,pkl->pij", E, T.transpose(0, 2, 1), optimize=True), Cv, eo, ev,
                                batch=4)


@pytest.mark.parametrize("N, n_occ, n_frozen", [(9, 3, 0), (12, 5, 1), (14, 6, 2), (10, 1, 0), (11, 4, 3)])
def test_terms_from_blocks_equal_restricted_terms_on_random_data(N, n_occ, n_frozen):
    """the last two cases: one occupied orbital, without and by freezing the others"""
    E, C, eps = _random_case(N, n_occ, 200 + N)
    got, S = _blocks_and_terms(E, C, eps, n_occ, n_frozen)
    want = mr.restricted_terms(E, C, eps, n_occ, n_frozen)
    for g, w, s in zip(got, want, S):
        assert abs(g - w) <= 1e-12 * abs(w), (got, want)
        assert s >= abs(w) * (1 - 1e-12)                              # (sum |x| bounds |sum x|)


@pytest.mark.parametrize("tag", ["n2_sto3g", "co_631g", "hf_ccpvdz", "ne_ccpvdz", "n2_ccpvdz"])
def test_terms_from_blocks_equal_restricted_terms_on_the_golden_systems(mp3_golden, tag):
    g = mp3_golden[tag]
    E = dense(tag)
    nocc = int(g["n_occ"])
    for nf in (0, 1, nocc - 1):
        got, S = _blocks_and_terms(E, g["C"], g["eps"], nocc, nf)
        want = mr.restricted_terms(E, g["C"], g["eps"], nocc, nf)
        assert np.all(np.abs(np.array(got) - np.array(want)) <= 1e-12 * np.abs(want)), (tag, nf, got, want)
        if nf < 2:
            assert abs(sum(got) - float(g[("", "fc1_")[nf] + "E_MP3"])) < 1e-10
