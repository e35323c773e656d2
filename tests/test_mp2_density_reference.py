"""CPU: the NumPy MP2 density of tests/mp2_density_reference.py against the reference program's own densities
(tests/golden/mp2_density_systems.npz, tools/make_golden_mp2_density.py): every element of the unrelaxed and the relaxed P in the MO and
the AO basis and of z within 1e-12, for MP2 and SCS-MP2 on all six systems; the trace, the symmetry, the natural occupations and the
dipole moment; and the conditioning the golden tool promises (cond(A + B) 1e-15 max|z| < 1e-11)."""
import numpy as np
import pytest

import mp2_density_reference as mr
from conftest import R_H2, R_N2
from tuna_amd import molecule as mol

SYSTEMS = {"h2_sto3g": (["H", "H"], R_H2, "STO-3G"), "co_sto3g": (["C", "O"], mol.angstrom_to_bohr(1.128), "STO-3G"),
           "co_631g": (["C", "O"], mol.angstrom_to_bohr(1.128), "6-31G"), "n2_ccpvdz": (["N", "N"], R_N2, "cc-pVDZ"),
           "n2_ccpvtz": (["N", "N"], R_N2, "cc-pVTZ"), "f2_631g": (["F", "F"], mol.angstrom_to_bohr(1.412), "6-31G")}
METHODS = ("mp2", "scs")
TOL = 1e-12


def split(z):
    out = {}
    for key in z.files:
        tag, name = key.split("__", 1)
        out.setdefault(tag, {})[name] = z[key]
    return out


def system(tag):
    sym, R, basis = SYSTEMS[tag]
    atoms = mol.make_atoms(sym, R)
    shells = mol.build_shells(atoms, basis)
    return atoms, shells, mol.expand_cartesian_aos(shells)


@pytest.fixture(scope="module")
def dens_golden(golden):
    return split(golden("mp2_density_systems"))


def test_golden_file_holds_the_systems(dens_golden):
    assert set(dens_golden) == set(SYSTEMS)
    shapes = {tag: (int(g["n_occ"]), len(g["eps"]) - int(g["n_occ"])) for tag, g in dens_golden.items()}
    assert shapes["h2_sto3g"] == (1, 1) and shapes["co_sto3g"][1] < shapes["co_sto3g"][0]
    assert shapes["f2_631g"][0] ** 2 > 64 and sum(shapes["f2_631g"]) <= 30 and sum(shapes["n2_ccpvtz"]) == 60
    for tag, g in dens_golden.items():
        for m in METHODS:
            assert float(g[f"{m}_cond"]) * 1e-15 * np.abs(g[f"{m}_z"]).max() < 1e-11, (tag, m)
    assert float(dens_golden["co_631g"]["scs_c_os"]) == 6 / 5 and float(dens_golden["co_631g"]["scs_c_ss"]) == 1 / 3


@pytest.mark.parametrize("tag", list(SYSTEMS))
def test_restatement_against_the_golden(dens_golden, tag):
    g = dens_golden[tag]
    _, shells, aos = system(tag)
    E = mr.dense_eri(aos, shells)
    C, eps, nocc = g["C"], g["eps"], int(g["n_occ"])
    gmo = mr.mo_integrals(E, C)
    for m in METHODS:
        c_os, c_ss = float(g[f"{m}_c_os"]), float(g[f"{m}_c_ss"])
        for kind in ("unrelaxed", "relaxed"):
            r = mr.mp2_density(E, C, eps, nocc, 0, kind == "relaxed", c_os, c_ss, g=gmo)
            d_mo = np.abs(r["P_mo"] - g[f"{m}_P_mo_{kind}"]).max()
            d_ao = np.abs(r["P_ao"] - g[f"{m}_P_ao_{kind}"]).max()
            d_z = np.abs(r["z"] - g[f"{m}_z"]).max() if kind == "relaxed" else 0.0
            d_e = max(abs(r["E_OS"] - float(g["E_OS"])), abs(r["E_SS"] - float(g["E_SS"])))
            print(f"\n[{tag} {m} {kind}] dP_mo {d_mo:.1e} dP_ao {d_ao:.1e} dz {d_z:.1e} dE {d_e:.1e}")
            assert d_mo < TOL and d_ao < TOL and d_z < TOL and d_e < TOL
            assert abs(np.trace(r["P_mo"]) - 2 * nocc) < 1e-11                      # tr P_mo = the number of electrons
            assert abs(np.sum(r["P_ao"] * g["S"]) - 2 * nocc) < 1e-11
            assert np.abs(r["P_mo"] - r["P_mo"].T).max() < 1e-14 and np.abs(r["P_ao"] - r["P_ao"].T).max() < 1e-13
            occ, orb = mr.natural_orbitals(r["P_ao"], g["X"])
            want = g[f"{m}_occ"] if kind == "relaxed" else g[f"{m}_occ_unrelaxed"]
            assert np.abs(occ - want).max() < 1e-11 and np.all(np.diff(occ) <= 1e-14)
            assert np.abs(orb.T @ g["S"] @ orb - np.eye(len(eps))).max() < 1e-11
            mu = g[f"{m}_dipole"] if kind == "relaxed" else g[f"{m}_dipole_unrelaxed"]
            assert abs(-np.sum(r["P_ao"] * g["dipz"]) - mu[2]) < 1e-11 and abs(mu[0] - (mu[1] + mu[2])) < 1e-14
        if nocc > 1:                                                               # (o = v = 1: z is zero by symmetry)
            assert np.abs(g[f"{m}_P_mo_relaxed"] - g[f"{m}_P_mo_unrelaxed"]).max() > 1e-3


def test_field_derivative_and_the_bound_of_the_gpu_test():
    """Independent of the reference program: for CO/6-31G, Tr(P_relaxed D_z) is dE/dF_z of E_RHF + E_MP2 (oracle/scf_oracle.py's cycle
    at EXTREME thresholds with F D_z in the core Hamiltonian, the four-point stencil).  The stencil at h = 0.004 and at h / 2 gives
    -0.08567957245 and -0.08567956854; ten times their difference, 3.9e-8, is the bound of tests/test_gpu_mp2_density.py, which this
    test derives again.  The relaxed density meets it, the unrelaxed one (+0.1509) does not."""
    from oracle import scf_oracle as so
    h, bound = 0.004, 3.9e-8
    atoms, shells, aos = system("co_631g")
    sd = mr.field_system(atoms, shells, aos)
    cache = {}

    def E(F):
        key = round(F / (h / 2))
        if key not in cache:
            cache[key] = mr.cpu_field_energy(sd, 7, F)
        return cache[key]
    d_h, d_half = mr.stencil(E, h), mr.stencil(E, h / 2)
    print(f"\n[co_631g] stencil at h {d_h:.11f} at h / 2 {d_half:.11f} ten times the difference {10 * abs(d_h - d_half):.2e}")
    assert abs(10 * abs(d_h - d_half) / bound - 1) < 0.05
    P0, E0 = so.core_guess(sd["T"], sd["V"], sd["X"], 7)
    r = so.run_rhf(sd["S"], sd["T"], sd["V"], sd["E"], sd["X"], P0, E0, 7, sd["V_NN"], sd["ranges"], conv="extreme")
    tr = {rel: float(np.sum(mr.mp2_density(sd["E"], r["C"], r["epsilons"], 7, 0, rel)["P_ao"] * sd["Dz"])) for rel in (True, False)}
    assert abs(tr[True] - d_h) < bound and abs(tr[True] - d_half) < bound
    assert not abs(tr[False] - d_h) < bound and abs(tr[False] - 0.1509) < 1e-4


def test_frozen_core_and_refusal(dens_golden):
    g = dens_golden["co_631g"]
    _, shells, aos = system("co_631g")
    E = mr.dense_eri(aos, shells)
    C, eps, nocc = g["C"], g["eps"], int(g["n_occ"])
    r = mr.mp2_density(E, C, eps, nocc, 1)
    assert abs(np.trace(r["P_mo"]) - 2 * nocc) < 1e-11
    assert np.all(r["P_mo"][0, 1:] == 0) and r["P_mo"][0, 0] == 2.0               # the frozen orbital keeps the reference determinant's 2
    with pytest.raises(ValueError):
        mr.mp2_density(E, C, eps, nocc, 1, relaxed=True)
