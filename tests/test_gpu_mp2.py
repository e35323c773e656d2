"""GPU: AO->MO transformation (rocBLAS f64 GEMMs on the resident tensor) and RMP2 energy -- BASELINE config 5 -- against the
reference's own transform_ERI_AO_to_MO / run_restricted_MP2 expressions (tests/golden/mp2_systems.npz)."""
import numpy as np
import pytest

from conftest import R_CO, make_system
from oracle import oracle as orc
from oracle import scf_oracle as so
from tuna_amd import molecule as mol

pytestmark = pytest.mark.gpu


def _system(tag):
    if tag == "co_631g":
        atoms = mol.make_atoms(["C", "O"], R_CO)
        shells = mol.build_shells(atoms, "6-31G")
        return atoms, shells, mol.expand_cartesian_aos(shells), 7
    return make_system({"n2_sto3g": "n2_sto3g", "n2_ccpvdz": "n2_ccpvdz", "c5_n2_ccpvtz": "c2_n2_ccpvtz"}[tag])


@pytest.mark.parametrize("tag", ["n2_sto3g", "n2_ccpvdz", "c5_n2_ccpvtz", "co_631g"])
def test_rmp2_energy_and_mo_integrals(engine, mp2_golden, tag):
    g = mp2_golden[tag]
    atoms, shells, aos, nocc = _system(tag)
    engine.set_basis(aos).build_eri(True)
    r = engine.mp2_rhf(g["C"], g["eps"], nocc)
    assert abs(r["E_OS"] - float(g["E_OS"])) < 1e-10 and abs(r["E_SS"] - float(g["E_SS"])) < 1e-10
    assert abs(r["E_MP2"] - (float(g["E_OS"]) + float(g["E_SS"]))) < 1e-10
    # the full (pq|rs) transformation, sampled against the reference tensor
    if engine.N <= 60:
        MO = engine.ao_to_mo(g["C"])
        idx = g["mo_idx"]
        assert np.abs(MO[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]] - g["mo_val"]).max() < 1e-11
        for perm in [(1, 0, 2, 3), (2, 3, 0, 1)]:
            assert np.abs(MO - MO.transpose(perm)).max() < 1e-11


def test_mixed_orbital_blocks_against_oracle(engine):
    """(i a | p q)-type transformation with four different coefficient blocks vs a NumPy einsum of the oracle tensor."""
    atoms, shells, aos, nocc = make_system("n2_sto3g")
    engine.set_basis(aos).build_eri(True)
    Es = so.eri_to_spherical(engine.sph_matrix(), orc.eri(aos))
    rng = np.random.default_rng(1)
    N = engine.N
    C1, C2, C3, C4 = rng.standard_normal((N, 3)), rng.standard_normal((N, 5)), rng.standard_normal((N, 2)), rng.standard_normal((N, N))
    ref = np.einsum("mnls,mp,nq,lr,st->pqrt", Es, C1, C2, C3, C4, optimize=True)
    assert np.abs(engine.ao_to_mo(C1, C2, C3, C4) - ref).max() < 1e-11


@pytest.mark.parametrize("n3", [1, 7, 16, 17, 18, 19, 20, 21, 31, 32, 33])
def test_first_quarter_kernel_against_the_einsum_and_the_block_path(engine, n3, monkeypatch):
    """tfmp2::mo_q1_kernel (hand-written MFMA-f64 first quarter on the packed segments, taken when the first ket coefficient matrix has at most
    32 columns): one and two column tiles, 17 - 20 columns (one tile + the vector-ALU columns), odd widths, the edge 32 | 33, against the NumPy einsum of the engine's own dense tensor (pinned
    to the oracle elsewhere) and against the expanded-block path (TF_MO_Q1=0) on N2/cc-pVTZ (N = 60, all four parity classes, f shells)."""
    atoms, shells, aos, nocc = make_system("c2_n2_ccpvtz")
    engine.set_basis(aos).build_eri(True)
    E = engine.copy_eri()
    rng = np.random.default_rng(10 + n3)
    N = engine.N
    C1, C2, C3, C4 = rng.standard_normal((N, 5)), rng.standard_normal((N, 9)), rng.standard_normal((N, n3)), rng.standard_normal((N, 11))
    ref = np.einsum("mnls,mp,nq,lr,st->pqrt", E, C1, C2, C3, C4, optimize=True)
    scale = np.abs(ref).max()
    monkeypatch.delenv("TF_MO_Q1", raising=False)
    fast = engine.ao_to_mo(C1, C2, C3, C4)
    assert np.abs(fast - ref).max() < 1e-12 * max(1.0, scale)
    monkeypatch.setenv("TF_MO_Q1", "0")
    blocks = engine.ao_to_mo(C1, C2, C3, C4)
    assert np.abs(blocks - ref).max() < 1e-12 * max(1.0, scale)
    assert np.abs(fast - blocks).max() < 1e-12 * max(1.0, scale)
    # the same matrices on both sides (the (ia|jb) case: one transformation serves both halves of the tensor)
    monkeypatch.delenv("TF_MO_Q1", raising=False)
    if n3 <= 18:
        same = engine.ao_to_mo(C3, C2, C3, C2)
        ref2 = np.einsum("mnls,mp,nq,lr,st->pqrt", E, C3, C2, C3, C2, optimize=True)
        assert np.abs(same - ref2).max() < 1e-12 * max(1.0, np.abs(ref2).max())


def test_first_quarter_kernel_with_wide_classes(engine, monkeypatch):
    """N = 200 (81 / 48 / 48 / 23 AOs per parity class): blocks of 16 output AOs per class in numbers, walks of several pipelined passes in
    both images, rows of every length.  The dense copy of the GPU tensor (pinned block-wise to the oracle by the parity tests) through the
    reference's einsum (tuna_ci.py:204-255, contracted in NumPy in a cheaper order) against tf_ao_to_mo on both paths."""
    counts = mol.synthetic_counts(200)
    atoms = mol.make_atoms(["AR", "AR"], 7.1)
    aos = mol.expand_cartesian_aos(mol.build_shells(atoms, {18: mol.even_tempered_basis(*counts)}))
    engine.set_basis(aos).build_eri(True, layout="packed")
    N = engine.N
    E = engine.copy_eri()
    rng = np.random.default_rng(5)
    C1, C2, C3, C4 = rng.standard_normal((N, 4)), rng.standard_normal((N, 6)), rng.standard_normal((N, 18)), rng.standard_normal((N, 7))
    t = np.tensordot(E, C3, axes=([2], [0]))                    # [m n s r]
    t = np.tensordot(t, C4, axes=([2], [0]))                    # [m n r t]
    t = np.tensordot(C1, t, axes=([0], [0]))                    # [p n r t]
    ref = np.tensordot(C2, t, axes=([0], [1])).transpose(1, 0, 2, 3)
    monkeypatch.delenv("TF_MO_Q1", raising=False)
    fast = engine.ao_to_mo(C1, C2, C3, C4)
    assert np.abs(fast - ref).max() < 1e-11 * np.abs(ref).max()
    monkeypatch.setenv("TF_MO_Q1", "0")
    assert np.abs(engine.ao_to_mo(C1, C2, C3, C4) - ref).max() < 1e-11 * np.abs(ref).max()
    monkeypatch.delenv("TF_MO_Q1", raising=False)
    Q, _ = np.linalg.qr(rng.standard_normal((N, N)))
    eps = np.concatenate([-np.arange(18, 0, -1.0), np.arange(1.0, N - 18 + 1)])
    r1 = engine.mp2_rhf(Q, eps, 18)
    monkeypatch.setenv("TF_MO_Q1", "0")
    r0 = engine.mp2_rhf(Q, eps, 18)
    assert abs(r1["E_OS"] - r0["E_OS"]) < 1e-10 * abs(r0["E_OS"]) and abs(r1["E_SS"] - r0["E_SS"]) < 1e-10 * abs(r0["E_SS"])


def test_scf_then_mp2_end_to_end(engine, mp2_golden):
    """Own orbitals (native RHF on the GPU) -> RMP2: total energy of BASELINE config 5, N2 MP2/cc-pVTZ."""
    from tuna_amd.energy import run
    g = mp2_golden["c5_n2_ccpvtz"]
    out = run("SPE : N N 1.0977 : HF CC-PVTZ : EXTREME", engine=engine)
    r = engine.mp2_rhf(out.molecular_orbitals, out.epsilons, 7)
    assert abs(out.energy - float(g["E_SCF"])) < 1e-9
    assert abs(r["E_MP2"] - (float(g["E_OS"]) + float(g["E_SS"]))) < 1e-8


def test_mp2_input_line(engine, mp2_golden):
    """The reference-style input line of BASELINE config 5: `SPE : N N 1.0977 : MP2 CC-PVTZ`."""
    from tuna_amd import energy
    g = mp2_golden["c5_n2_ccpvtz"]
    lines = []
    out = energy.run("SPE : N N 1.0977 : MP2 CC-PVTZ : EXTREME", silent=False, engine=engine, log=lines.append)
    e_corr = float(g["E_OS"]) + float(g["E_SS"])
    assert abs(out.correlation_energy_mp2 - e_corr) < 1e-8
    assert abs(out.energy - (float(g["E_SCF"]) + e_corr)) < 1e-8
    text = "\n".join(lines)
    assert "MP2 correlation energy:" in text and "Final single point energy:" in text


def _mp2_numpy(E, C, eps, n_occ, n_frozen=0):
    """(E_OS, E_SS) from the dense spherical tensor E (tuna_ci.py:204-255 restricted to (ia|jb), tuna_mp.py:882-890)"""
    Co, Cv = C[:, n_frozen:n_occ], C[:, n_occ:]
    g = np.einsum("mnls,mi,na,lj,sb->iajb", E, Co, Cv, Co, Cv, optimize=True)
    eo, ev = eps[n_frozen:n_occ], eps[n_occ:]
    D = eo[:, None, None, None] - ev[None, :, None, None] + eo[None, None, :, None] - ev[None, None, None, :]
    return float(np.sum(g * g / D)), float(np.sum(g * (g - g.transpose(0, 3, 2, 1)) / D))


@pytest.fixture(scope="module")
def n2_tz_oracle(engine):
    atoms, shells, aos, nocc = make_system("c2_n2_ccpvtz")
    engine.set_basis(aos)
    return aos, so.eri_to_spherical(engine.sph_matrix(), orc.eri(aos))


@pytest.mark.parametrize("n_occ", [1, 16, 17, 20, 21, 32, 33, 40])
def test_rmp2_occupied_widths_against_the_oracle_tensor(engine, n2_tz_oracle, n_occ):
    """tf_mp2_rhf with 1 - 40 occupied orbitals on N2/cc-pVTZ (N = 60): one and two MFMA column tiles of the first quarter, the vector-ALU
    columns (17, 20), the edge 32 | 33 where the energy moves to the expanded-block path, against NumPy on the oracle tensor; random
    orthonormal orbitals, occupied and virtual energies separated by a gap."""
    aos, E = n2_tz_oracle
    engine.set_basis(aos).build_eri(True)
    N = engine.N
    rng = np.random.default_rng(60 + n_occ)
    C = np.linalg.qr(rng.standard_normal((N, N)))[0]
    eps = np.concatenate([np.sort(rng.uniform(-4.0, -0.6, n_occ)), np.sort(rng.uniform(0.3, 8.0, N - n_occ))])
    r = engine.mp2_rhf(C, eps, n_occ)
    e_os, e_ss = _mp2_numpy(E, C, eps, n_occ)
    assert abs(r["E_OS"] - e_os) <= 1e-10 and abs(r["E_SS"] - e_ss) <= 1e-10, (r, e_os, e_ss)


def test_rmp2_frozen_core_and_bad_arguments(engine, mp2_golden, n2_tz_oracle):
    """Frozen core (n_frozen 1, 2, 6 of the 7 occupied orbitals of N2/cc-pVTZ, reference orbitals) against NumPy on the oracle tensor; the
    arguments tf_mp2_rhf refuses (n_frozen < 0, n_frozen = n_occ, n_occ >= N) raise TF_EINVAL and leave the context usable."""
    from tuna_amd._lib import TunaError
    g = mp2_golden["c5_n2_ccpvtz"]
    aos, E = n2_tz_oracle
    engine.set_basis(aos).build_eri(True)
    N = engine.N
    C, eps = g["C"], g["eps"]
    r0 = engine.mp2_rhf(C, eps, 7)
    assert abs(r0["E_OS"] - float(g["E_OS"])) < 1e-10 and abs(r0["E_SS"] - float(g["E_SS"])) < 1e-10
    for nf in (1, 2, 6):
        r = engine.mp2_rhf(C, eps, 7, nf)
        e_os, e_ss = _mp2_numpy(E, C, eps, 7, nf)
        assert abs(r["E_OS"] - e_os) <= 1e-10 and abs(r["E_SS"] - e_ss) <= 1e-10, (nf, r, e_os, e_ss)
        assert r["E_MP2"] > r0["E_MP2"]                                        # (freezing removes negative pair energies)
    for n_occ, nf in ((7, -1), (7, 7), (8, 9), (N, 0), (N + 3, 1)):
        with pytest.raises(TunaError) as ei:
            engine.mp2_rhf(C, eps, n_occ, nf)
        assert ei.value.code == -1, (n_occ, nf, ei.value.code)                # TF_EINVAL
    r1 = engine.mp2_rhf(C, eps, 7)
    assert r1["E_OS"] == r0["E_OS"] and r1["E_SS"] == r0["E_SS"]


@pytest.mark.parametrize("layout", ["tiles", "rows"])
def test_rmp2_energy_and_mo_integrals_on_other_layouts(engine, mp2_golden, layout):
    """As test_rmp2_energy_and_mo_integrals (N2/cc-pVTZ against the reference goldens), on the tiles layout and on the rows layout of one
    rank; the shared context gets the default layout back."""
    g = mp2_golden["c5_n2_ccpvtz"]
    atoms, shells, aos, nocc = _system("c5_n2_ccpvtz")
    try:
        engine.set_basis(aos).build_eri(True, layout=layout)
        assert engine.eri_storage()["layout"] == layout
        r = engine.mp2_rhf(g["C"], g["eps"], nocc)
        MO = engine.ao_to_mo(g["C"])
    finally:
        engine._check(engine._L.tf_set_eri_layout(engine._ctx, -1))
    assert abs(r["E_OS"] - float(g["E_OS"])) < 1e-10 and abs(r["E_SS"] - float(g["E_SS"])) < 1e-10
    idx = g["mo_idx"]
    assert np.abs(MO[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]] - g["mo_val"]).max() < 1e-11
    for perm in [(1, 0, 2, 3), (2, 3, 0, 1)]:
        assert np.abs(MO - MO.transpose(perm)).max() < 1e-11
