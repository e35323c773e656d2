"""CPU: the independent NumPy unrestricted CIS / TDHF and orbital-Hessian spectra of tests/ucis_reference.py against the reference
program's own numbers (tests/golden/ucis_systems.npz: the UHF orbitals of ump2_systems.npz) and against the restricted checker: CIS by
eigh, TDHF through the full non-symmetric problem and through the Cholesky reduction the library uses, the transition moments without
sqrt(2), the lowest Hessian eigenvalue from eig(A + B) and eig(A - B) against the reference's Hessian of order 2 dim, and the identity
C_alpha = C_beta = closed-shell RHF orbitals, where the unrestricted states are the merged singlets and triplets.

Which systems have a TDHF golden: the symmetric reduction exists where A + B and A - B are positive definite.  O2/STO-3G's UHF solution is
a saddle point (lowest Hessian eigenvalue -0.263, lowest CIS energy -0.261): marked unstable.  NO/6-31G and OH/cc-pVDZ have a zero mode
(|lowest| < 1e-12, the rotation of the singly occupied pi orbital): marked marginal, and only their CIS is compared.  O2/cc-pVDZ (all
electrons and with four frozen spin orbitals), Li/6-31G and H/cc-pVDZ are stable.

Deviation of the Cholesky route from the golden (the reference's eig of the 2 dim problem), the largest over all states of the stable
systems, measured here on the CPU: 2.8e-13 Eh (O2/cc-pVDZ, all electrons; the full route 6.8e-13 Eh); CIS against its eigh: 3.6e-14 Eh.
UTDHF_TOL is ten times the former and is the bound of the GPU tests as well."""
import numpy as np
import pytest

import cis_reference as cr
import ucis_reference as ur
from test_cis_reference import CIS_TOL, MOMENT_TOL, TDHF_TOL, cluster_sums, split
from test_cis_reference import system as closed_system
from tuna_amd import molecule as mol

A = mol.angstrom_to_bohr
SYSTEMS = {"o2_triplet_sto3g": (["O", "O"], A(1.2075), "STO-3G"), "o2_triplet_ccpvdz": (["O", "O"], A(1.2075), "cc-pVDZ"),
           "no_doublet_631g": (["N", "O"], A(1.1508), "6-31G"), "oh_doublet_ccpvdz": (["O", "H"], A(0.9697), "cc-pVDZ"),
           "li_doublet_631g": (["LI"], None, "6-31G"), "h_ccpvdz": (["H"], None, "cc-pVDZ")}
VARIANTS = {"o2_triplet_ccpvdz": (0, 4)}          # frozen spin orbitals, half of either spin
UNSTABLE = ("o2_triplet_sto3g",)
MARGINAL = ("no_doublet_631g", "oh_doublet_ccpvdz")
UTDHF_TOL = 2.8e-12                # Eh per state: ten times the measured deviation of the Cholesky route from the golden
STAB_TOL = 1e-10                   # lowest Hessian eigenvalue: eigvalsh of symmetric matrices of order <= 742 with entries <= 20, ~1e-13
RSTAB = ("n2_sto3g", "n2_ccpvdz", "n2_ccpvtz", "co_631g", "hf_ccpvdz", "ne_ccpvdz", "h2_sto3g", "h2_sto3g_2p0")
# (n_alpha, n_beta, frozen per spin) of the element-by-element test on N2/cc-pVTZ (N = 60) and what each is there for
RANDOM_CASES = [(1, 0, 0), (2, 1, 0), (8, 7, 0), (7, 8, 0), (8, 7, 1)]


def usystem(tag):
    sym, R, basis = SYSTEMS[tag]
    atoms = mol.make_atoms(sym, R)
    shells = mol.build_shells(atoms, basis)
    return shells, mol.expand_cartesian_aos(shells)


def variants(tag):
    return VARIANTS.get(tag, (0,))


def windows(g, k=0):
    """(n_alpha, n_beta, n_frozen_alpha, n_frozen_beta) of the variant with k frozen spin orbitals"""
    return int(g["n_alpha"]), int(g["n_beta"]), k // 2, k // 2


def orbitals(g):
    return g["C_alpha"], g["C_beta"], g["eps_alpha"], g["eps_beta"]


def random_uhf_orbitals(N, n_alpha, n_beta):
    """Random orthonormal orbitals of either spin with the energy ladder of test_gpu_mp3._random_orbitals (the beta one stretched by 3 %),
    the virtual energies of alpha 1.0 Eh and of beta 1.2 Eh higher.  With these shifts the checker finds, for every case of RANDOM_CASES,
    min eig(A - B) > 1.3, min w^2 > 1.6 and the six lowest CIS and TDHF states more than 1e-2 Eh apart
    (test_random_orbitals_are_stable_and_separated asserts it)."""
    rng = np.random.default_rng(1000 + 16 * n_alpha + n_beta)
    Ca = np.linalg.qr(rng.standard_normal((N, N)))[0]
    Cb = np.linalg.qr(rng.standard_normal((N, N)))[0]
    ladder = np.concatenate([-np.linspace(20.0, 0.5, 24), np.linspace(0.3, 8.0, N - 24)])
    ea, eb = ladder.copy(), 1.03 * ladder
    ea[n_alpha:] += 1.0
    eb[n_beta:] += 1.2
    return Ca, Cb, ea, eb


@pytest.fixture(scope="module")
def ucis_golden(golden):
    return split(golden("ucis_systems"))


@pytest.fixture(scope="module")
def n2_tz_dense():
    shells, aos = closed_system("n2_ccpvtz")
    return aos, cr.dense_eri(aos, shells)


def test_tolerances_are_below_the_input_line_tolerance():
    assert UTDHF_TOL < 1e-8 and CIS_TOL < 1e-8 and STAB_TOL < 1e-5


def test_golden_file_holds_the_systems(ucis_golden):
    assert set(ucis_golden) == set(SYSTEMS) | {"rstab"}
    stable = 0
    for tag in SYSTEMS:
        g = ucis_golden[tag]
        N = len(g["eps_alpha"])
        for k in variants(tag):
            na, nb, nfa, nfb = windows(g, k)
            dim = sum(ur.dims(N, na, nb, nfa, nfb))
            assert len(g[f"CIS_fc{k}_energies"]) == len(g[f"CIS_fc{k}_tdm"]) == len(g[f"CIS_fc{k}_osc"]) == dim
            assert (f"TDHF_fc{k}_unstable" in g) == (tag in UNSTABLE) and (f"TDHF_fc{k}_marginal" in g) == (tag in MARGINAL)
            assert (f"TDHF_fc{k}_energies" in g) == (tag not in UNSTABLE + MARGINAL)
            if tag in UNSTABLE:
                assert g[f"stab_fc{k}_lowest"] < -1e-5
            elif tag in MARGINAL:
                assert abs(g[f"stab_fc{k}_lowest"]) < 1e-6
            else:
                assert g[f"stab_fc{k}_lowest"] > 1e-6 and len(g[f"TDHF_fc{k}_energies"]) == dim
                stable += k == 0
    assert stable >= 3
    for tag in RSTAB:
        assert f"{tag}__singlet" in ucis_golden["rstab"] and f"{tag}__triplet" in ucis_golden["rstab"]


@pytest.mark.parametrize("tag", list(SYSTEMS))
def test_checker_against_the_golden(ucis_golden, tag):
    g = ucis_golden[tag]
    shells, aos = usystem(tag)
    E = cr.dense_eri(aos, shells)
    Ca, Cb, ea, eb = orbitals(g)
    for k in variants(tag):
        na, nb, nfa, nfb = windows(g, k)
        da, db = ur.dims(len(ea), na, nb, nfa, nfb)
        m = ur.matrices(E, Ca, Cb, ea, eb, na, nb, nfa, nfb)
        assert np.array_equal(m["A"], m["A"].T) and np.array_equal(m["B"], m["B"].T)
        assert not m["minus"][:da, da:].any() and not m["minus"][da:, :da].any()          # (ia alpha|jb beta) cancels exactly in A - B
        # the Hessian's spectrum is eig(A + B) u eig(A - B): against the matrix of order 2 dim and against the reference's lowest
        spectra, lowest = ur.hessian_spectra_uhf(m)
        full = ur.full_hessian_lowest(m["A"], m["B"])
        d_stab = abs(lowest - float(g[f"stab_fc{k}_lowest"]))
        print(f"\n[{tag} fc{k}] d_alpha {da} d_beta {db} lowest Hessian eigenvalue {lowest:.8f} (order 2 dim: d {abs(lowest - full):.1e}; golden: d {d_stab:.1e})")
        assert abs(lowest - full) < STAB_TOL and d_stab < STAB_TOL
        e, V = ur.cis(m["A"])
        d_cis = np.abs(e - g[f"CIS_fc{k}_energies"]).max()
        _, mag, f = ur.transition_moments(g["dip"], Ca, Cb, na, nb, nfa, nfb, V, e)
        ge = g[f"CIS_fc{k}_energies"]
        d_mu = np.abs(cluster_sums(ge, mag) - cluster_sums(ge, g[f"CIS_fc{k}_tdm"])).max()
        d_f = np.abs(cluster_sums(ge, f) - cluster_sums(ge, g[f"CIS_fc{k}_osc"])).max()
        print(f"[{tag} fc{k}] CIS d {d_cis:.1e} cluster |mu| d {d_mu:.1e} f d {d_f:.1e}")
        assert d_cis < CIS_TOL and d_mu < MOMENT_TOL and d_f < MOMENT_TOL
        r = ur.tdhf_cholesky(m["plus"], m["minus"])
        if tag in UNSTABLE:
            assert e[0] < 0 and (r["E"] is None or r["min_w2"] < 0)
            continue
        if tag in MARGINAL:
            continue
        want = g[f"TDHF_fc{k}_energies"]
        w, X, Y = ur.tdhf_full(m["A"], m["B"])
        d_chol, d_full = np.abs(r["E"] - want).max(), np.abs(w - want).max()
        print(f"[{tag} fc{k}] TDHF Cholesky d {d_chol:.1e} full d {d_full:.1e} min eig(A - B) {r['min_eig_minus']:.4f} min w^2 {r['min_w2']:.6f}")
        assert d_chol < UTDHF_TOL and d_full < UTDHF_TOL and r["min_eig_minus"] > 0 and r["min_w2"] > 0
        assert np.abs(np.sum(r["X"] ** 2 - r["Y"] ** 2, axis=0) - 1).max() < 1e-12
        _, mag, f = ur.transition_moments(g["dip"], Ca, Cb, na, nb, nfa, nfb, r["X"] + r["Y"], r["E"])
        d_mu = np.abs(cluster_sums(want, mag) - cluster_sums(want, g[f"TDHF_fc{k}_tdm"])).max()
        d_f = np.abs(cluster_sums(want, f) - cluster_sums(want, g[f"TDHF_fc{k}_osc"])).max()
        print(f"[{tag} fc{k}] TDHF cluster |mu| d {d_mu:.1e} f d {d_f:.1e}")
        assert d_mu < MOMENT_TOL and d_f < MOMENT_TOL


@pytest.mark.parametrize("tag", ["co_631g", "hf_ccpvdz", "n2_sto3g"])
def test_identity_with_the_restricted_checker(golden, tag):
    """C_alpha = C_beta = closed-shell RHF orbitals: the unrestricted CIS / TDHF energies are the merged singlets and triplets of the
    restricted checker, the oscillator strengths agree by clusters, and the lowest Hessian eigenvalue is min(singlet, triplet)."""
    g = split(golden("cis_systems"))[tag]
    shells, aos = closed_system(tag)
    E = cr.dense_eri(aos, shells)
    C, eps, nocc = g["C"], g["eps"], int(g["n_occ"])
    mr = cr.matrices(E, C, eps, nocc, 0)
    mu = ur.matrices(E, C, C, eps, eps, nocc, nocc)
    es, Vs = cr.cis(mr["A_singlet"])
    et = cr.cis(mr["A_triplet"])[0]
    e, V = ur.cis(mu["A"])
    assert np.abs(e - np.sort(np.concatenate([es, et]))).max() < CIS_TOL
    _, mag_r, f_r = cr.transition_moments(g["dip"], C, nocc, 0, Vs, es)
    merged_e, _, _, merged_f = cr.merged(es, et, mag_r, f_r)
    _, _, f_u = ur.transition_moments(g["dip"], C, C, nocc, nocc, 0, 0, V, e)
    assert np.abs(cluster_sums(merged_e, f_u) - cluster_sums(merged_e, merged_f)).max() < MOMENT_TOL
    spectra, ls, lt = ur.hessian_spectra_rhf(E, C, eps, nocc)
    _, lowest = ur.hessian_spectra_uhf(mu)
    assert abs(lowest - min(ls, lt)) < STAB_TOL
    assert np.abs(np.sort(np.concatenate([spectra["plus_singlet"], spectra["plus_triplet"]])) - np.linalg.eigvalsh(mu["plus"])).max() < 1e-10
    rs, rt = cr.tdhf_cholesky(mr["plus_singlet"], mr["minus"]), cr.tdhf_cholesky(mr["plus_triplet"], mr["minus"])
    if rs["E"] is not None and rs["min_w2"] > 0 and rt["min_w2"] > 0:
        r = ur.tdhf_cholesky(mu["plus"], mu["minus"])
        assert np.abs(r["E"] - np.sort(np.concatenate([rs["E"], rt["E"]]))).max() < TDHF_TOL


def test_restricted_stability_against_the_golden(ucis_golden):
    """The lowest singlet and triplet Hessian eigenvalues of the reference for the closed-shell molecules, and stretched H2: at 2.0
    angstrom the singlet Hessian is positive and the triplet one negative, w^2 / (A - B) = -0.0473 / 0.1184 = -0.3999."""
    rs = ucis_golden["rstab"]
    cis = split(np.load(__import__("os").path.join(__import__("conftest").GOLD, "cis_systems.npz")))
    for tag in RSTAB:
        if tag.startswith("h2_sto3g"):
            R = A(2.0) if tag.endswith("2p0") else A(0.74)
            aos, E, C, eps = cr.h2_minimal_basis(R)
            nocc = 1
        else:
            shells, aos = closed_system(tag)
            E = cr.dense_eri(aos, shells)
            C, eps, nocc = cis[tag]["C"], cis[tag]["eps"], int(cis[tag]["n_occ"])
        _, ls, lt = ur.hessian_spectra_rhf(E, C, eps, nocc)
        print(f"\n[{tag}] lowest singlet {ls:.8f} triplet {lt:.8f} (golden {float(rs[tag + '__singlet']):.8f} {float(rs[tag + '__triplet']):.8f})")
        assert abs(ls - float(rs[f"{tag}__singlet"])) < STAB_TOL and abs(lt - float(rs[f"{tag}__triplet"])) < STAB_TOL
    aos, E, C, eps = cr.h2_minimal_basis(A(2.0))
    m = cr.matrices(E, C, eps, 1, 0)
    _, ls, lt = ur.hessian_spectra_rhf(E, C, eps, 1)
    assert abs(ls - m["minus"][0, 0]) < 1e-15 and abs(ls - 0.11839) < 1e-5 and abs(lt - m["plus_triplet"][0, 0]) < 1e-15 and abs(lt + 0.39988) < 1e-5
    assert abs(lt - cr.tdhf_cholesky(m["plus_triplet"], m["minus"])["min_w2"] / m["minus"][0, 0]) < 1e-12


@pytest.mark.parametrize("na,nb,nf", RANDOM_CASES)
def test_random_orbitals_are_stable_and_separated(n2_tz_dense, na, nb, nf):
    """What the GPU's element-by-element test relies on, for every case it runs."""
    aos, E = n2_tz_dense
    N = E.shape[0]
    Ca, Cb, ea, eb = random_uhf_orbitals(N, na, nb)
    m = ur.matrices(E, Ca, Cb, ea, eb, na, nb, nf, nf)
    r = ur.tdhf_cholesky(m["plus"], m["minus"])
    e = ur.cis(m["A"])[0]
    k = min(6, len(e))
    gaps = min(np.diff(e[:k]).min(), np.diff(r["E"][:k]).min()) if k > 1 else np.inf
    print(f"\n[{na} {nb} frozen {nf}] dims {ur.dims(N, na, nb, nf, nf)} min eig(A - B) {r['min_eig_minus']:.3f} min w^2 {r['min_w2']:.3f} smallest gap {gaps:.2e}")
    assert r["min_eig_minus"] > 0.9 and r["min_w2"] > 0.8 and gaps > 1e-3      # (measured: 1.30, 1.69, 1.0e-2 at the least)
