"""CPU: the independent NumPy CIS / TDHF of tests/cis_reference.py against the reference program's own states
(tests/golden/cis_systems.npz) and against itself: CIS by eigh, TDHF through the full 2 dim non-symmetric problem and through the Cholesky
reduction the library uses, the matrices through integral-direct products with no MO block, the transition moments, and the unstable
references (N2/STO-3G's core-guess solution, stretched H2).

Deviation of the Cholesky route from the golden (the reference's eig of the 2 dim problem), the largest over all states of the six stable
systems, frozen 0 and 1, measured here on the CPU: 3.6e-13 Eh (N2/cc-pVTZ); CIS against its eigh: 5.0e-14 Eh.  TDHF_TOL is ten times the
former and is the bound of the GPU tests as well; it must stay below the 1e-8 Eh of the input-line tests."""
import numpy as np
import pytest

import cis_reference as cr
from conftest import R_H2, R_N2
from tuna_amd import molecule as mol

SYSTEMS = {"n2_sto3g": (["N", "N"], R_N2, "STO-3G"), "n2_ccpvdz": (["N", "N"], R_N2, "cc-pVDZ"), "n2_ccpvtz": (["N", "N"], R_N2, "cc-pVTZ"),
           "co_631g": (["C", "O"], mol.angstrom_to_bohr(1.128), "6-31G"), "hf_ccpvdz": (["F", "H"], mol.angstrom_to_bohr(0.917), "cc-pVDZ"),
           "ne_ccpvdz": (["NE"], None, "cc-pVDZ"), "h2_sto3g": (["H", "H"], R_H2, "STO-3G")}
UNSTABLE = ("n2_sto3g",)          # the reference's RHF solution from the core guess: negative CIS energies, A - B not positive definite
CIS_TOL = 1e-10                   # Eh per state
TDHF_TOL = 3.6e-12                # Eh per state: ten times the measured deviation of the Cholesky route from the golden
MOMENT_TOL = 1e-6                 # cluster sums of |mu| and f: ||dM|| <= 1e-11 over the smallest gap between clusters, 5.8e-5 Eh, times |mu| <= 2
R_H2_UNSTABLE = mol.angstrom_to_bohr(2.0)


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
    return shells, mol.expand_cartesian_aos(shells)


def frozen_variants(g):
    return (0, 1) if int(g["n_occ"]) > 1 else (0,)


def cluster_sums(golden_energies, values):
    return np.array([np.sum(values[c]) for c in cr.clusters(golden_energies)])


@pytest.fixture(scope="module")
def cis_golden(golden):
    return split(golden("cis_systems"))


def test_tdhf_tolerance_is_below_the_input_line_tolerance():
    assert TDHF_TOL < 1e-8 and CIS_TOL < 1e-8


def test_golden_file_holds_the_systems(cis_golden):
    assert set(cis_golden) == set(SYSTEMS)
    for tag, g in cis_golden.items():
        for nf in frozen_variants(g):
            dim = (int(g["n_occ"]) - nf) * (len(g["eps"]) - int(g["n_occ"]))
            assert len(g[f"CIS_fc{nf}_E_singlet"]) == len(g[f"CIS_fc{nf}_E_triplet"]) == dim
            assert (f"TDHF_fc{nf}_unstable" in g) == (tag in UNSTABLE)
            for method in ("CIS",) + (() if tag in UNSTABLE else ("TDHF",)):
                pre = f"{method}_fc{nf}_"
                e, lab = g[pre + "energies"], g[pre + "labels"]
                assert len(e) == 2 * dim and np.all(np.diff(e) >= 0) and np.array_equal(np.sort(e[lab == 0]), g[pre + "E_singlet"])
                assert np.all(g[pre + "tdm"][lab == 1] == 0) and np.all(g[pre + "osc"][lab == 1] == 0)


@pytest.mark.parametrize("tag", list(SYSTEMS))
def test_three_forms_against_the_golden(cis_golden, tag):
    g = cis_golden[tag]
    shells, aos = system(tag)
    E = cr.dense_eri(aos, shells)
    C, eps, nocc = g["C"], g["eps"], int(g["n_occ"])
    rng = np.random.default_rng(5)
    for nf in frozen_variants(g):
        m = cr.matrices(E, C, eps, nocc, nf)
        o, v = nocc - nf, len(eps) - nocc
        scale = max(np.abs(m[k]).max() for k in cr.KINDS)
        # the matrices against integral-direct products with random trial vectors
        b = rng.standard_normal((3, o, v))
        direct = cr.direct_products(E, C, eps, nocc, nf, b)
        for kind in cr.KINDS:
            d = np.abs(direct[kind].reshape(3, -1) - b.reshape(3, -1) @ m[kind]).max()
            assert d < 1e-11 * scale * np.sqrt(o * v), (tag, nf, kind, d)
        stable = tag not in UNSTABLE
        for mult in ("singlet", "triplet"):
            e, V = cr.cis(m[f"A_{mult}"])
            d_cis = np.abs(e - g[f"CIS_fc{nf}_E_{mult}"]).max()
            r = cr.tdhf_cholesky(m[f"plus_{mult}"], m["minus"])
            if not stable:
                print(f"\n[{tag} fc{nf} {mult}] CIS d {d_cis:.1e} lowest {e[0]:.6f}; min eig(A - B) {r['min_eig_minus']:.4f}: unstable")
                assert d_cis < CIS_TOL and e[0] < 0 and r["min_eig_minus"] < 0 and r["E"] is None
                continue
            want = g[f"TDHF_fc{nf}_E_{mult}"]
            w, X, Y = cr.tdhf_full(m[f"A_{mult}"], m[f"B_{mult}"])
            d_chol, d_full = np.abs(r["E"] - want).max(), np.abs(w - want).max()
            print(f"\n[{tag} fc{nf} {mult}] CIS d {d_cis:.1e} TDHF Cholesky d {d_chol:.1e} full d {d_full:.1e} min eig(A - B) {r['min_eig_minus']:.4f} "
                  f"min w^2 {r['min_w2']:.4f}")
            assert d_cis < CIS_TOL and d_chol < TDHF_TOL and d_full < TDHF_TOL
            assert r["min_eig_minus"] > 0 and r["min_w2"] > 0 and len(w) == o * v
            assert np.abs(np.sum(r["X"] ** 2 - r["Y"] ** 2, axis=0) - 1).max() < 1e-12
            assert np.abs(np.sum(X ** 2 - Y ** 2, axis=0) - 1).max() < 1e-12
        # transition moments of the merged list, by clusters of degenerate states
        for method in ("CIS",) + (("TDHF",) if stable else ()):
            pre = f"{method}_fc{nf}_"
            if method == "CIS":
                Es, XpY = cr.cis(m["A_singlet"])
                Et = cr.cis(m["A_triplet"])[0]
            else:
                rs, rt = cr.tdhf_cholesky(m["plus_singlet"], m["minus"]), cr.tdhf_cholesky(m["plus_triplet"], m["minus"])
                Es, XpY, Et = rs["E"], rs["X"] + rs["Y"], rt["E"]
            _, mag, f = cr.transition_moments(g["dip"], C, nocc, nf, XpY, Es)
            e, lab, mu, osc = cr.merged(Es, Et, mag, f)
            ge = g[pre + "energies"]
            d_mu = np.abs(cluster_sums(ge, mu) - cluster_sums(ge, g[pre + "tdm"])).max()
            d_f = np.abs(cluster_sums(ge, osc) - cluster_sums(ge, g[pre + "osc"])).max()
            print(f"[{tag} fc{nf} {method}] cluster sums: |mu| d {d_mu:.1e} f d {d_f:.1e} sum f {osc.sum():.6f}")
            assert d_mu < MOMENT_TOL and d_f < MOMENT_TOL


def test_stretched_h2_is_triplet_unstable():
    """H2/STO-3G at 2.0 angstrom, past the Coulson-Fischer point (1.2 angstrom in this basis): A - B > 0 but the triplet A + B < 0, so the
    triplet w^2 = -0.0473 < 0 while the singlet w^2 = 0.0754 > 0; the lowest CIS triplet is -0.1407 Eh."""
    aos, E, C, eps = cr.h2_minimal_basis(R_H2_UNSTABLE)
    m = cr.matrices(E, C, eps, 1, 0)
    rs, rt = cr.tdhf_cholesky(m["plus_singlet"], m["minus"]), cr.tdhf_cholesky(m["plus_triplet"], m["minus"])
    print(f"\nmin eig(A - B) {rt['min_eig_minus']:.6f} triplet w^2 {rt['min_w2']:.6f} singlet w^2 {rs['min_w2']:.6f} CIS triplet {m['A_triplet'][0, 0]:.6f}")
    assert rt["min_eig_minus"] > 0.1 and rt["min_w2"] < -0.04 and rs["min_w2"] > 0.07 and m["A_triplet"][0, 0] < -0.14
    assert np.isnan(rt["E"][0]) and abs(rs["E"][0] - np.sqrt(rs["min_w2"])) < 1e-15
    # at equilibrium the same construction reproduces the golden's H2 (whose orbitals come from the reference's SCF)
    aos, E, C, eps = cr.h2_minimal_basis(R_H2)
    m = cr.matrices(E, C, eps, 1, 0)
    assert abs(m["A_triplet"][0, 0] - 0.5859859424546581) < 1e-10 and abs(m["A_singlet"][0, 0] - 0.9484068652448535) < 1e-10
