"""GPU: the MP2 one-particle density on the resident tensor (tf_mp2_density_rhf: the amplitude, Lagrangian and assembly kernels of
tf_mp2dens.hip.h, the AO-direct ladder with the occupied back-transformation, the J/K build, the assembly pass of tf_cis.hip.h, rocSOLVER
dpotrf / dpotrs) and the natural orbitals (tf_natural_orbitals) against the reference program's own densities
(tests/golden/mp2_density_systems.npz), the NumPy restatement of tests/mp2_density_reference.py and a derivative of the library's own
energies.  Every test hands the shared context back with the default layout.

The tolerance of the golden comparison is the 1e-10 of tests/test_gpu_mp2.py on every element of P in both bases, on z and on the
energies.  Measured on one MI355X, the largest over the six systems, both methods, both kinds and the three layouts: 3.3e-15 (P, MO
basis), 6.5e-14 (P, AO basis), 6.6e-15 (z), 8.5e-15 Eh (energies), all at N2/cc-pVTZ; natural occupations 1.7e-14, orthonormality 1.2e-13;
the dipole moments of the two input lines 3.1e-10 and 4.6e-10; the field derivative 4.1e-9 against its bound of 3.9e-8."""
import numpy as np
import pytest

import mp2_density_reference as mr
from test_gpu_mp3 import _reset
from test_mp2_density_reference import METHODS, SYSTEMS, split, system
from tuna_amd import energy
from tuna_amd._lib import TunaError

pytestmark = pytest.mark.gpu

TF_ELINALG = -5
TOL = 1e-10                        # |dP| per element (MO and AO), |dz| per element, |dE|: the criterion of tests/test_gpu_mp2.py
DIPOLE_TOL = 1e-9                  # input lines against the golden dipole moment
LAYOUT_SYSTEMS = ("co_631g", "n2_ccpvdz", "f2_631g")
# the derivative test (test_relaxed_density_is_the_field_derivative has the derivation)
FIELD_H = 0.004
FIELD_BOUND = 3.9e-8


@pytest.fixture(scope="module")
def dens_golden(golden):
    return split(golden("mp2_density_systems"))


def compare(engine, g, m, relaxed):
    """(dP_mo, dP_ao, dz, dE) of one call against the golden, and the result"""
    kind = "relaxed" if relaxed else "unrelaxed"
    r = engine.mp2_density_rhf(g["C"], g["eps"], int(g["n_occ"]), 0, relaxed=relaxed, c_os=float(g[f"{m}_c_os"]), c_ss=float(g[f"{m}_c_ss"]))
    d = [np.abs(r["P_mo"] - g[f"{m}_P_mo_{kind}"]).max(), np.abs(r["P_ao"] - g[f"{m}_P_ao_{kind}"]).max(),
         np.abs(r["z"] - g[f"{m}_z"]).max() if relaxed else 0.0, max(abs(r["E_OS"] - float(g["E_OS"])), abs(r["E_SS"] - float(g["E_SS"])))]
    return d, r


@pytest.mark.parametrize("tag", list(SYSTEMS))
def test_golden_parity(engine, dens_golden, tag):
    """Every golden system on the packed layout, MP2 and SCS-MP2, unrelaxed and relaxed: every element of P in both bases, z and the
    energies within 1e-10; the trace is the number of electrons and P is symmetric.  o = v = 1 (H2), v < o (CO/STO-3G), all four
    parity classes (N2/cc-pVTZ), a full and a ragged batch of the ladder (F2/6-31G, 81 pairs)."""
    g = dens_golden[tag]
    engine.set_basis(system(tag)[2]).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed"
    bad = []
    for m in METHODS:
        for relaxed in (False, True):
            d, r = compare(engine, g, m, relaxed)
            print(f"\n[{tag} {m} {'relaxed' if relaxed else 'unrelaxed'}] dP_mo {d[0]:.1e} dP_ao {d[1]:.1e} dz {d[2]:.1e} dE {d[3]:.1e} seconds {r['seconds']}")
            if not max(d) < TOL:
                bad.append((m, relaxed, d))
            assert abs(np.trace(r["P_mo"]) - 2 * int(g["n_occ"])) < 1e-10
            assert np.array_equal(r["P_mo"], r["P_mo"].T) and np.abs(r["P_ao"] - r["P_ao"].T).max() < 1e-12
            assert (r["L"] is None and r["z"] is None) if not relaxed else r["L"].shape == r["z"].shape
    assert not bad, bad


@pytest.mark.parametrize("layout", ["rows", "tiles"])
def test_other_layouts(engine, dens_golden, layout):
    """CO/6-31G, N2/cc-pVDZ and F2/6-31G on the rows and tiles layouts, where the ladder goes through the general-density exchange build
    and the back-transformation has one image: the same tolerance."""
    bad = []
    try:
        for tag in LAYOUT_SYSTEMS:
            g = dens_golden[tag]
            engine.set_basis(system(tag)[2]).build_eri(True, layout=layout)
            assert engine.eri_storage()["layout"] == layout
            for m in METHODS:
                for relaxed in (False, True):
                    d, _ = compare(engine, g, m, relaxed)
                    print(f"\n[{layout} {tag} {m} {'relaxed' if relaxed else 'unrelaxed'}] dP_mo {d[0]:.1e} dP_ao {d[1]:.1e} dz {d[2]:.1e} dE {d[3]:.1e}")
                    if not max(d) < TOL:
                        bad.append((tag, m, relaxed, d))
    finally:
        _reset(engine)
    assert not bad, bad


def test_energies_of_mp2_rhf_and_a_second_call(engine, dens_golden):
    """N2/cc-pVDZ: E_OS and E_SS are those of mp2_rhf within 1e-12, and a second relaxed call returns the same bits in every array."""
    g = dens_golden["n2_ccpvdz"]
    engine.set_basis(system("n2_ccpvdz")[2]).build_eri(True)
    args = (g["C"], g["eps"], int(g["n_occ"]), 0)
    e = engine.mp2_rhf(*args)
    a = engine.mp2_density_rhf(*args, relaxed=True, c_os=1.2, c_ss=1 / 3)
    b = engine.mp2_density_rhf(*args, relaxed=True, c_os=1.2, c_ss=1 / 3)
    assert abs(a["E_OS"] - e["E_OS"]) < 1e-12 and abs(a["E_SS"] - e["E_SS"]) < 1e-12
    for k in ("E_OS", "E_SS", "P_mo", "P_ao", "L", "z"):
        assert np.array_equal(a[k], b[k]), k
    u = engine.mp2_density_rhf(*args)
    assert np.array_equal(u["P_mo"], engine.mp2_density_rhf(*args)["P_mo"])
    o = slice(0, int(g["n_occ"]))
    assert np.array_equal(u["P_mo"][o, o], engine.mp2_density_rhf(*args, relaxed=True)["P_mo"][o, o])


def test_frozen_orbitals(engine, dens_golden):
    """CO/6-31G with one frozen orbital: the unrelaxed density is the NumPy restatement's within 1e-10 (the golden file is all-electron),
    the frozen orbital keeps its 2; relaxed with a frozen orbital is refused, in Python and by the library."""
    import ctypes
    from tuna_amd._lib import Mp2DensityOpts, Mp2DensityResult, ptr
    g = dens_golden["co_631g"]
    _, shells, aos = system("co_631g")
    engine.set_basis(aos).build_eri(True)
    C, eps, nocc = g["C"], g["eps"], int(g["n_occ"])
    ref = mr.mp2_density(mr.dense_eri(aos, shells), C, eps, nocc, 1, False, 1.2, 1 / 3)
    r = engine.mp2_density_rhf(C, eps, nocc, 1, c_os=1.2, c_ss=1 / 3)
    d = max(np.abs(r["P_mo"] - ref["P_mo"]).max(), np.abs(r["P_ao"] - ref["P_ao"]).max(), abs(r["E_OS"] - ref["E_OS"]), abs(r["E_SS"] - ref["E_SS"]))
    print(f"\n[co_631g fc1] d {d:.1e}")
    assert d < TOL and r["P_mo"][0, 0] == 2.0 and np.all(r["P_mo"][0, 1:] == 0)
    with pytest.raises(TunaError, match="n_frozen = 0"):
        engine.mp2_density_rhf(C, eps, nocc, 1, relaxed=True)
    P = np.zeros((len(eps), len(eps)))
    res = Mp2DensityResult()
    res.P_mo = ptr(P)
    opts = Mp2DensityOpts(1, 1.0, 1.0)
    Cc, ec = np.ascontiguousarray(C), np.ascontiguousarray(eps)
    assert engine._L.tf_mp2_density_rhf(engine._ctx, ctypes.byref(opts), nocc, 1, ptr(Cc), ptr(ec), ctypes.byref(res)) == -1
    assert b"n_frozen = 0" in engine._L.tf_last_error(engine._ctx)
    for bad in ((C[:, :-1], eps, nocc, 0), (C, eps[:-1], nocc, 0), (C, eps, len(eps), 0), (C, eps, nocc, nocc), (C, eps, nocc, -1)):
        with pytest.raises(TunaError):
            engine.mp2_density_rhf(*bad)


@pytest.mark.parametrize("tag", list(SYSTEMS))
def test_natural_orbitals(engine, dens_golden, tag):
    """Occupations of the golden relaxed and unrelaxed densities within 1e-10 of the reference's, descending, summing to the electron
    count; the orbitals are S-orthonormal and rebuild P.  Orbitals are not compared one by one: pi pairs are degenerate."""
    g = dens_golden[tag]
    S, X, n_el = g["S"], g["X"], 2 * int(g["n_occ"])
    for m in METHODS:
        for kind, key in (("relaxed", f"{m}_occ"), ("unrelaxed", f"{m}_occ_unrelaxed")):
            P = g[f"{m}_P_ao_{kind}"]
            occ, orb = engine.natural_orbitals(P, X)
            d_occ = np.abs(occ - g[key]).max()
            d_orth = np.abs(orb.T @ S @ orb - np.eye(len(occ))).max()
            d_P = np.abs((orb * occ) @ orb.T - P).max()
            print(f"\n[{tag} {m} {kind}] d occ {d_occ:.1e} orthonormality {d_orth:.1e} rebuilt P {d_P:.1e}")
            assert d_occ < TOL and np.all(np.diff(occ) <= 0) and abs(np.sum(occ) - n_el) < 1e-10
            assert d_orth < 1e-10 and d_P < TOL


def test_singlet_instability_is_an_error_return(engine, golden):
    """N2/STO-3G with HOMO and LUMO exchanged in C and eps: a negative diagonal of A + B, dpotrf stops, TF_ELINALG; the context works on."""
    z = golden("mp3_systems")
    C, eps, nocc = z["n2_sto3g__C"].copy(), z["n2_sto3g__eps"].copy(), int(z["n2_sto3g__n_occ"])
    from test_cis_reference import system as cis_system
    engine.set_basis(cis_system("n2_sto3g")[1]).build_eri(True)
    C[:, [nocc - 1, nocc]] = C[:, [nocc, nocc - 1]]
    eps[[nocc - 1, nocc]] = eps[[nocc, nocc - 1]]
    with pytest.raises(TunaError, match="not positive definite.*singlet-unstable") as e:
        engine.mp2_density_rhf(C, eps, nocc, 0, relaxed=True)
    assert e.value.code == TF_ELINALG
    u = engine.mp2_density_rhf(C, eps, nocc, 0)               # the unrelaxed density of the same orbitals needs no solve
    assert abs(np.trace(u["P_mo"]) - 2 * nocc) < 1e-10


def _run(line, engine):
    lines = []
    out = energy.run(line, silent=False, engine=engine, log=lambda s="": lines.append(str(s)))
    return out, "\n".join(lines) + "\n"


@pytest.mark.parametrize("line,m,kind", [("SPE : C O 1.128 : MP2 6-31G : RELAXED NATORBS", "mp2", "relaxed"),
                                         ("SPE : C O 1.128 : SCS-MP2 6-31G : UNRELAXED NATORBS", "scs", "unrelaxed")])
def test_input_lines(engine, dens_golden, line, m, kind):
    """The whole path from the input line: the golden dipole moment (total, nuclear, electronic) within 1e-9, the reference's
    "Constructing ..." line and natural-occupation block as printed, the "Using ..." line, and the fields of the output."""
    g = dens_golden["co_631g"]
    out, text = _run(line, engine)
    mu = g[f"{m}_dipole"] if kind == "relaxed" else g[f"{m}_dipole_unrelaxed"]
    got = np.array(out.properties["dipole_moment"])
    print(f"\n[{line}] dipole {got} golden {mu} d {np.abs(got - mu).max():.1e}")
    assert np.abs(got - mu).max() < DIPOLE_TOL
    assert str(g[f"text_{m}_{kind}"]) in text, text
    assert f"\n Using the MP2 {kind} density for property calculations.\n" in text
    occ = g[f"{m}_occ"] if kind == "relaxed" else g[f"{m}_occ_unrelaxed"]
    assert np.abs(out.natural_orbital_occupancies - occ).max() < DIPOLE_TOL
    assert np.array_equal(out.P_alpha, out.P / 2) and np.array_equal(out.P_beta, out.P / 2)
    assert abs(np.sum(out.P * out.S) - 14) < 1e-9 and out.mp2["P_mo"].shape == out.P.shape and out.natural_orbitals.shape == out.P.shape
    assert (out.mp2["z"] is not None) == (kind == "relaxed")


def test_a_line_without_the_keywords_prints_what_it_printed(engine):
    """MP2 and SCS-MP2 lines without RELAXED / UNRELAXED / NATORBS: no density work, no new line, no new field."""
    for method in ("MP2", "SCS-MP2"):
        out, text = _run(f"SPE : C O 1.128 : {method} 6-31G", engine)
        assert "density" not in text.lower() and "Natural orbital" not in text
        assert not hasattr(out, "natural_orbital_occupancies") and "P_mo" not in out.mp2 and "MP2 density" not in out.timings
        plain, _ = _run("SPE : C O 1.128 : HF 6-31G", engine)
        assert np.abs(out.P - plain.P).max() < 1e-6           # still the Hartree-Fock density
        with_density, text2 = _run(f"SPE : C O 1.128 : {method} 6-31G : UNRELAXED", engine)
        # the same text, with the density's two messages taken out where they stand
        own = ("\n  Constructing MP2 unrelaxed density...      [Done]\n", "\n Using the MP2 unrelaxed density for property calculations.\n")
        assert all(text2.count(s) == 1 for s in own)
        assert text2.replace(own[0], "").replace(own[1], "") == text
        assert with_density.energy == out.energy


def test_relaxed_density_is_the_field_derivative(engine, dens_golden):
    """Independent of the reference program: for CO/6-31G, Tr(P_relaxed D_z) from mp2_density_rhf is dE/dF_z of E_RHF + E_MP2, the
    derivative taken from Engine.scf_rhf(Fext = F D_z) at EXTREME thresholds plus mp2_rhf with the four-point stencil at h and 2h.
    h = 0.004 a.u.  The bound is not tuned on the device: tests/test_mp2_density_reference.py computes the same stencil on the CPU
    (oracle/scf_oracle.py's cycle and the NumPy MP2) at h and h / 2, -0.08567957245 and -0.08567956854, and the bound is ten times
    their difference, 10 x 3.9e-9 = 3.9e-8: the truncation error of the stencil at h (it falls as h^4: 6.3e-8 between 2h and h) with
    an order of magnitude for the convergence noise of the cycles.  The unrelaxed density (Tr = +0.1509) must miss the same bound."""
    calc = energy.Calculation("SPE", "HF", "6-31G")
    atoms = system("co_631g")[0]
    molecule, integrals, X, guess, _ = energy.build_molecule_and_integrals(["C", "O"], atoms[1].origin[2], calc, engine)
    from tuna_amd import molecule as mol
    V_NN, nocc, Dz = mol.nuclear_repulsion(molecule.atoms), molecule.n_doubly_occ, integrals.D[2]

    def E(F):
        r = engine.scf_rhf(integrals.S, integrals.T, integrals.V_NE, guess[0], guess[3], nocc, V_NN, X=X, Fext=F * Dz, conv="extreme",
                           n_atom_ao=molecule.partition_ranges)
        assert r["converged"]
        return r["energy"] + engine.mp2_rhf(r["C"], r["epsilons"], nocc, 0)["E_MP2"], r
    derivative = mr.stencil(lambda F: E(F)[0], FIELD_H)
    _, r0 = E(0.0)
    relaxed = engine.mp2_density_rhf(r0["C"], r0["epsilons"], nocc, 0, relaxed=True)
    unrelaxed = engine.mp2_density_rhf(r0["C"], r0["epsilons"], nocc, 0)
    tr_r, tr_u = float(np.sum(relaxed["P_ao"] * Dz)), float(np.sum(unrelaxed["P_ao"] * Dz))
    print(f"\n[co_631g] dE/dF {derivative:.11f} Tr(P_relaxed D_z) {tr_r:.11f} d {abs(tr_r - derivative):.1e} (bound {FIELD_BOUND:.1e}) "
          f"Tr(P_unrelaxed D_z) {tr_u:.11f}")
    assert abs(tr_r - derivative) < FIELD_BOUND
    assert not abs(tr_u - derivative) < FIELD_BOUND
    d = dens_golden["co_631g"]["mp2_dipole"]
    assert abs(-tr_r - d[2]) < DIPOLE_TOL                     # the electronic dipole moment of the golden file
