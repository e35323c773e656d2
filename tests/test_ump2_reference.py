"""CPU: the independent UMP2 of tests/ump2_reference.py against the reference program's own run_unrestricted_MP2
(tests/golden/ump2_systems.npz, tools/make_golden_ump2.py) on the golden orbitals, frozen-core variants included.
tests/test_gpu_ump2.py then judges the library by it."""
import numpy as np
import pytest

import ump2_reference as ur
from conftest import make_uhf_system
from tuna_amd import molecule as mol

EXTRA = {"h_ccpvdz": (["H"], None, "cc-pVDZ"), "o2_triplet_ccpvtz": (["O", "O"], mol.angstrom_to_bohr(1.2075), "cc-pVTZ")}


@pytest.fixture(scope="module")
def ump2_golden(golden):
    z = golden("ump2_systems")
    out = {}
    for key in z.files:
        tag, name = key.split("__", 1)
        out.setdefault(tag, {})[name] = z[key]
    return out


def system(tag):
    if tag in EXTRA:
        sym, R, basis = EXTRA[tag]
        atoms = mol.make_atoms(sym, R)
        shells = mol.build_shells(atoms, basis)
        return shells, mol.expand_cartesian_aos(shells)
    _, shells, aos, _, _ = make_uhf_system(tag)
    return shells, aos


@pytest.mark.parametrize("tag", ["o2_triplet_sto3g", "o2_triplet_ccpvdz", "no_doublet_631g", "oh_doublet_ccpvdz", "li_doublet_631g",
                                 "h_ccpvdz", "o2_triplet_ccpvtz"])
def test_checker_matches_reference_goldens(ump2_golden, tag):
    g = ump2_golden[tag]
    shells, aos = system(tag)
    E = ur.dense_eri(aos, shells)
    na, nb = int(g["n_alpha"]), int(g["n_beta"])
    args = (E, g["C_alpha"], g["C_beta"], g["eps_alpha"], g["eps_beta"], na, nb)
    got = ur.pair_energies(*args)
    for k, name in enumerate(("E_aa", "E_bb", "E_ab")):
        assert abs(got[k] - float(g[name])) < 1e-11, (tag, name, got[k], float(g[name]))
    for kf in (2, 3):
        if f"fc{kf}_E_aa" not in g:
            continue
        fa, fb = ur.frozen_split(kf)
        got = ur.pair_energies(*args, n_frozen_alpha=fa, n_frozen_beta=fb)
        for k, name in enumerate(("E_aa", "E_bb", "E_ab")):
            assert abs(got[k] - float(g[f"fc{kf}_{name}"])) < 1e-11, (tag, kf, name, got[k], float(g[f"fc{kf}_{name}"]))


def test_closed_shell_limit_matches_scs_golden(ump2_golden):
    """N2/cc-pVTZ (closed shell): the reference's USCS-MP2 energy is 1/3 E_SS + 6/5 E_OS of the pair energies."""
    g = ump2_golden["n2_ccpvtz"]
    assert abs(float(g["E_aa"]) - float(g["E_bb"])) < 1e-12
    scs = (float(g["E_aa"]) + float(g["E_bb"])) / 3 + 1.2 * float(g["E_ab"])
    assert abs(scs - float(g["scs_E_MP2"])) < 1e-12
