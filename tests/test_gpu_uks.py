"""GPU: unrestricted Kohn-Sham -- tf_dft_vxc_unrestricted (spin-resolved V_XC, tuna_amd/csrc/tf_dft.hip.h) and tf_scf_uks (the native
unrestricted cycle with V_XC^alpha, V_XC^beta) against the reference's own unrestricted runs (tests/golden/uks_systems.npz,
tools/make_golden_uks.py) and against the independent spin-polarised CPU reference of tests/xc_reference_spin.py; the closed-shell
limit against the restricted path; V_XC as the gradient of E_XC; the input line; the error paths and bitwise repeatability."""
import ctypes
import os

import numpy as np
import pytest

import xc_reference as xr
import xc_reference_spin as xs
from tuna_amd import molecule as mol
from tuna_amd._lib import TunaError, ptr

pytestmark = pytest.mark.gpu

TF_EINVAL = -1
PAIRS = [(x, c) for x in range(4) for c in range(6) if x or c]
TOL_V, TOL_E = 2e-14, 5e-12                 # whole grids: the bars of test_gpu_dft_reference.py (V relative to max|V|; integrals relative)


@pytest.fixture(scope="module")
def uks(golden):
    z = golden("uks_systems")
    out = {}
    for key in z.files:
        tag, name = key.split("__", 1)
        out.setdefault(tag, {})[name] = z[key]
    return out


def _spec(tag):
    """(symbols, R in bohr or None, basis, n_alpha, n_beta, functional, grid) of a golden system, as stored with it."""
    from conftest import GOLD
    g = np.load(os.path.join(GOLD, "uks_systems.npz"))
    R = float(g[tag + "__R"])
    return ([str(x) for x in g[tag + "__symbols"]], None if np.isnan(R) else R, str(g[tag + "__basis"]), int(g[tag + "__n_alpha"]),
            int(g[tag + "__n_beta"]), str(g[tag + "__functional"]), str(g[tag + "__grid"]))


TAGS = ["o2_b3lyp_sto3g", "o2_svwn_sto3g", "o2_b3lyp_ccpvdz", "o2_svwn_ccpvdz", "no_blyp_631g", "oh_b3lypg_ccpvdz", "li_svwn3_631g",
        "h_b3lyp_ccpvdz", "nh_hfs_sto3g", "nh_hfb_sto3g", "nh_bvwn_sto3g", "nh_bvwn3_sto3g", "nh_bhlyp_sto3g", "nh_b1lyp_sto3g",
        "nh_slyp_sto3g"]


def _setup(engine, tag):
    from tuna_amd import dft
    sym, R, basis, na, nb, method, grid = _spec(tag)
    atoms = mol.make_atoms(sym, R)
    shells = mol.build_shells(atoms, basis)
    aos = mol.expand_cartesian_aos(shells)
    engine.set_basis(aos).build_eri(True)
    pts, wts, info = dft.integration_grid(atoms, grid)
    f = engine.dft_setup(pts, wts, method)
    return atoms, shells, aos, na, nb, f, (np.asarray(pts).reshape(3, -1), np.asarray(wts).reshape(-1))


def _vxcu_rc(engine, Pa, Pb):
    Pa, Pb = np.ascontiguousarray(Pa, dtype=np.float64), np.ascontiguousarray(Pb, dtype=np.float64)
    Va, Vb = np.zeros_like(Pa), np.zeros_like(Pb)
    n, ex, ec = np.zeros(2), np.zeros(2), ctypes.c_double()
    dp = ctypes.POINTER(ctypes.c_double)
    rc = engine._L.tf_dft_vxc_unrestricted(engine._ctx, ptr(Pa), ptr(Pb), ptr(Va), ptr(Vb), n.ctypes.data_as(dp), ex.ctypes.data_as(dp),
                                           ctypes.byref(ec))
    return rc, Va, Vb, n, ex, ec.value


# ---- 1. guess densities against the reference ---------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", TAGS)
def test_vxc_of_guess_densities(engine, uks, tag):
    g = uks[tag]
    _setup(engine, tag)
    Va, Vb, n, ex, ec = engine.dft_vxc_unrestricted(g["P0_alpha"], g["P0_beta"])
    engine.dft_clear()
    err = max(np.abs(Va - g["V_XC0_alpha"]).max(), np.abs(Vb - g["V_XC0_beta"]).max(), *np.abs(np.array(n) - g["n0"]),
              *np.abs(np.array(ex) - g["EX0"]), abs(ec - float(g["EC0"])))
    print(f"MEASURED guess {tag}: {err:.2e}")
    assert err < 1e-9
    assert np.abs(Va - Va.T).max() == 0.0 and np.abs(Vb - Vb.T).max() == 0.0


# ---- 2. against the independent spin reference ----------------------------------------------------------------------------------

def _random_psd(rng, N, k, scale):
    C = rng.standard_normal((N, k))
    return scale * (C @ C.T) / k


def test_random_densities_every_functional_pair(engine):
    """Random PSD alpha / beta densities over the whole O2 / STO-3G grid for every (x, c) id pair."""
    from tuna_amd import dft
    from tuna_amd.spherical import transformation_matrix
    atoms = mol.make_atoms(["O", "O"], mol.angstrom_to_bohr(1.2075))
    shells = mol.build_shells(atoms, "STO-3G")
    aos = mol.expand_cartesian_aos(shells)
    engine.set_basis(aos).build_eri(True)
    U = transformation_matrix([s.L for s in shells])
    pts, wts, _ = dft.integration_grid(atoms, "loose")
    pts, wts = np.asarray(pts).reshape(3, -1), np.asarray(wts).reshape(-1)
    grid = xr.ao_grid(aos, pts, U)
    rng = np.random.default_rng(11)
    N = engine.N
    Pa, Pb = _random_psd(rng, N, 6, 0.3), _random_psd(rng, N, 4, 0.2)
    worst = [0.0, 0.0]
    for xid, cid in PAIRS:
        dfx, dfc = 0.8, 1.0
        pts_c, wts_c = np.ascontiguousarray(pts), np.ascontiguousarray(wts)
        assert engine._L.tf_dft_setup(engine._ctx, wts.size, ptr(pts_c), ptr(wts_c), xid, cid, dfx, dfc, 2.0 / 3.0) == 0
        rc, Va, Vb, n, ex, ec = _vxcu_rc(engine, Pa, Pb)
        assert rc == 0
        Var, Vbr, nr, exr, ecr = xs.vxc_unrestricted(aos, pts, wts, Pa, Pb, xid, cid, dfx, dfc, grid=grid)
        eV = max(np.abs(Va - Var).max() / np.abs(Var).max(), np.abs(Vb - Vbr).max() / np.abs(Vbr).max())
        eE = max(abs(a - b) / abs(b) for a, b in zip([*n, *ex, ec], [*nr, *exr, ecr]) if b != 0.0)
        print(f"MEASURED random ({xid},{cid}): V {eV:.2e} E {eE:.2e}")
        worst = [max(worst[0], eV), max(worst[1], eE)]
        assert eV < TOL_V and eE < TOL_E, (xid, cid, eV, eE)
    engine.dft_clear()
    print(f"MEASURED random worst: V {worst[0]:.2e} E {worst[1]:.2e}")


_O2_POOL = {}


def _o2_pool(engine):
    """O2 / STO-3G on the engine; the AOs, U and the loose grid's points with w > 1e-6 within 4 bohr of the bond midpoint (computed once)."""
    from tuna_amd import dft
    from tuna_amd.spherical import transformation_matrix
    atoms = mol.make_atoms(["O", "O"], mol.angstrom_to_bohr(1.2075))
    shells = mol.build_shells(atoms, "STO-3G")
    aos = mol.expand_cartesian_aos(shells)
    engine.set_basis(aos).build_eri(True)
    if not _O2_POOL:
        pts, wts, _ = dft.integration_grid(atoms, "loose")
        pts, wts = np.asarray(pts).reshape(3, -1), np.asarray(wts).reshape(-1)
        mid = 0.5 * (np.asarray(atoms[0].origin, dtype=float) + np.asarray(atoms[1].origin, dtype=float))
        r = np.sqrt(((pts - mid[:, None]) ** 2).sum(axis=0))
        keep = np.flatnonzero((wts > 1e-6) & (r < 4.0))
        _O2_POOL.update(pts=pts, wts=wts, keep=keep, U=transformation_matrix([s.L for s in shells]))
    return aos, _O2_POOL


@pytest.mark.parametrize("G", [1, 127, 128, 129, 256, 128 * 3 + 5])
def test_split_k_branches_unrestricted(engine, G):
    """The 2N-wide V assembly at its split-K edges, as test_gpu_dft_reference.py::test_split_k_branches pins the restricted one: real
    points and weights of O2 / STO-3G (N = 10, loose grid; those with w > 1e-6 within 4 bohr of the bond midpoint, in the random order of
    default_rng(G), so that the remainder rows are as significant as the others) cut to G points: G < 128 runs only the remainder GEMM, a
    multiple of 128 no remainder GEMM, the others both.  B3LYP ids, random PSD densities, against xc_reference_spin; V_alpha, V_beta
    exactly symmetric; a second call gives the same bits.  Bars: TOL_V and TOL_E of the whole grids.  Measured worst on the build
    before the two assemblies were folded into one and on the one after, the same figures: V 6.8e-16 (G = 1), integrals 7.2e-16 (G = 1)."""
    aos, pool = _o2_pool(engine)
    assert pool["wts"].size == 28196 and pool["keep"].size == 8680
    idx = np.random.default_rng(G).permutation(pool["keep"])[:G]
    assert idx.size == G
    pts, wts = np.ascontiguousarray(pool["pts"][:, idx]), np.ascontiguousarray(pool["wts"][idx])
    N = engine.N
    assert N == 10
    rng = np.random.default_rng(11)
    Pa, Pb = _random_psd(rng, N, 6, 0.3), _random_psd(rng, N, 4, 0.2)
    xid, cid, dfx, dfc = 3, 4, 0.8, 1.0                                         # B3LYP: B3 exchange, 3P (VWN5) correlation
    assert engine._L.tf_dft_setup(engine._ctx, G, ptr(pts), ptr(wts), xid, cid, dfx, dfc, 2.0 / 3.0) == 0
    rc, Va, Vb, n, ex, ec = _vxcu_rc(engine, Pa, Pb)
    again = _vxcu_rc(engine, Pa, Pb)
    engine.dft_clear()
    assert rc == 0 and again[0] == 0
    Var, Vbr, nr, exr, ecr = xs.vxc_unrestricted(aos, pts, wts, Pa, Pb, xid, cid, dfx, dfc, grid=xr.ao_grid(aos, pts, pool["U"]))
    eV = max(np.abs(Va - Var).max() / np.abs(Var).max(), np.abs(Vb - Vbr).max() / np.abs(Vbr).max())
    eE = max(abs(a - b) / abs(b) for a, b in zip([*n, *ex, ec], [*nr, *exr, ecr]) if b != 0.0)
    print(f"MEASURED split-K unrestricted G={G}: V {eV:.2e} E {eE:.2e}")
    assert eV < TOL_V and eE < TOL_E, (G, eV, eE)
    assert np.abs(Va - Va.T).max() == 0.0 and np.abs(Vb - Vb.T).max() == 0.0
    assert np.array_equal(Va, again[1]) and np.array_equal(Vb, again[2])
    assert np.array_equal(n, again[3]) and np.array_equal(ex, again[4]) and ec == again[5]


SP_BASIS = {7: [("S", [(0.9, 1.0)]), ("P", [(0.6, 1.0)])]}


def _point_densities():
    """(label, P_alpha, P_beta) on the s / p_z block of one N atom at a point on the z axis: rho_beta on the floor, zeta = +1 and -1,
    negative sigma_ab (opposite s-p_z couplings), very large and very small densities."""
    def blk(s, pz, c):
        P = np.zeros((4, 4))
        P[0, 0], P[3, 3], P[0, 3], P[3, 0] = s, pz, c, c
        return P
    A, B, Bneg = blk(1.0, 0.5, 0.3), blk(0.4, 0.2, 0.1), blk(0.4, 0.2, -0.25)
    Z = np.zeros((4, 4))
    return [("beta_floor", A, Z), ("zeta_plus", A, A * 1e-30), ("zeta_minus", Z, B), ("neg_sigma_ab", A, Bneg),
            ("large", A * 1e4, B * 1e4), ("small", A * 1e-12, Bneg * 1e-12), ("tiny_beta", A, B * 1e-14), ("near_closed", A, A * 0.999)]


def test_single_point_extremes_every_functional_pair(engine):
    """G = 1 on one N atom (s and p shells), the point on the z axis: every id pair at the spin edges.  Each V entry relative to the
    largest |V| entry of its matrix."""
    atoms = mol.make_atoms(["N"], None)
    shells = mol.build_shells(atoms, SP_BASIS)
    aos = mol.expand_cartesian_aos(shells)
    engine.set_basis(aos).build_eri(True)
    from tuna_amd.spherical import transformation_matrix
    U = transformation_matrix([s.L for s in shells])
    pt = np.array([[0.0], [0.0], [0.7]])
    w = np.array([0.37])
    grid = xr.ao_grid(aos, pt, U)
    worst = 0.0
    for xid, cid in PAIRS:
        assert engine._L.tf_dft_setup(engine._ctx, 1, ptr(np.ascontiguousarray(pt)), ptr(w), xid, cid, 0.8, 1.0, 2.0 / 3.0) == 0
        for label, Pa, Pb in _point_densities():
            rc, Va, Vb, n, ex, ec = _vxcu_rc(engine, Pa, Pb)
            assert rc == 0
            Var, Vbr, nr, exr, ecr = xs.vxc_unrestricted(aos, pt, w, Pa, Pb, xid, cid, 0.8, 1.0, grid=grid)
            eV = max(np.abs(Va - Var).max() / max(np.abs(Var).max(), 1e-300), np.abs(Vb - Vbr).max() / max(np.abs(Vbr).max(), 1e-300))
            eE = max([abs(a - b) / abs(b) for a, b in zip([*n, *ex, ec], [*nr, *exr, ecr]) if b != 0.0] + [0.0])
            # VWN: below rho = 1e-12 the formula cancels in double (the restricted bar, test_gpu_dft_reference.py); near zeta = +-1 the
            # kernel forms (1 -+ zeta)^(1/3) from a rounded zeta, as the reference does, where xc_reference_spin uses 2 rho_s / rho
            vwn = cid in (1, 2, 4, 5)
            tol = 1e-9 if vwn and label == "small" else 1e-5 if vwn and label in ("beta_floor", "zeta_plus", "zeta_minus", "tiny_beta") else 1e-13
            loose = tol > 1e-13
            print(f"MEASURED point ({xid},{cid}) {label}: V {eV:.2e} E {eE:.2e}")
            worst = max(worst, 0.0 if loose else eV)
            assert eV < tol and eE < tol, (xid, cid, label, eV, eE)
    engine.dft_clear()
    print(f"MEASURED point worst (outside the VWN edges): {worst:.2e}")


# ---- 3. closed-shell limit ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ["o2_b3lyp_sto3g", "o2_svwn_ccpvdz", "nh_slyp_sto3g", "nh_bhlyp_sto3g"])
def test_closed_shell_limit(engine, uks, tag):
    """P_alpha = P_beta = P / 2: V^alpha = V^beta = the restricted V_XC(P) and the energies add up (densities above the floors)."""
    g = uks[tag]
    _setup(engine, tag)
    P = g["P0_alpha"] + g["P0_beta"]
    V, n_el, exr, ecr = engine.dft_vxc(P)
    Va, Vb, n, ex, ec = engine.dft_vxc_unrestricted(P / 2, P / 2)
    engine.dft_clear()
    scale = np.abs(V).max()
    eV = max(np.abs(Va - V).max(), np.abs(Vb - V).max()) / scale
    eE = max(abs(n[0] + n[1] - n_el) / n_el, abs(ex[0] + ex[1] - exr) / abs(exr), abs(ec - ecr) / max(abs(ecr), 1e-300) if ecr else 0.0)
    print(f"MEASURED closed-shell limit {tag}: V {eV:.2e} E {eE:.2e}")
    assert eV < 1e-12 and eE < 1e-11


# ---- 4. V_XC as the gradient of E_XC -------------------------------------------------------------------------------------------

def test_vxc_is_the_gradient_of_exc(engine, uks):
    """(E_XC(P_s + hD) - E_XC(P_s - hD)) / 2h = <V^s, D> at a converged O2 triplet density (B3LYP / STO-3G), h = 1e-5: catches wrong
    factors on the sigma_ss and sigma_ab terms."""
    tag = "o2_b3lyp_sto3g"
    g = uks[tag]
    atoms, shells, aos, na, nb, f, _ = _setup(engine, tag)
    xyz, chg = [a.origin for a in atoms], [float(a.charge) for a in atoms]
    S, T, V, _, _ = engine.one_electron(xyz, chg, [0, 0, 0.0])
    X, _, _ = engine.orthogonaliser(S)
    ranges = [sum(s.n_sph for s in shells if s.atom == a) for a in range(len(atoms))]
    r = engine.scf_uks(S, T, V, g["P0_alpha"], g["P0_beta"], float(g["E0"]), na, nb, mol.nuclear_repulsion(atoms), X=X, conv="extreme",
                       damping="dynamic", hfx=f["hfx"], n_atom_ao=ranges, max_iter=int(g["max_iter"]))
    Pa, Pb = r["P_spin"]
    rng = np.random.default_rng(3)
    Dm = rng.standard_normal(Pa.shape)
    Dm = 0.5 * (Dm + Dm.T)
    h = 1e-5

    def exc(A, B):
        _, _, _, ex, ec = engine.dft_vxc_unrestricted(A, B)
        return ex[0] + ex[1] + ec
    Va, Vb, _, _, _ = engine.dft_vxc_unrestricted(Pa, Pb)
    for s, (A, B, Vs) in enumerate(((Pa, Pb, Va), (Pa, Pb, Vb))):
        plus = exc(A + h * Dm, B) if s == 0 else exc(A, B + h * Dm)
        minus = exc(A - h * Dm, B) if s == 0 else exc(A, B - h * Dm)
        fd = (plus - minus) / (2 * h)
        an = float(np.sum(Vs * Dm))
        rel = abs(fd - an) / abs(an)
        print(f"MEASURED gradient spin {s}: fd {fd:.12e} analytic {an:.12e} rel {rel:.2e}")
        assert rel < 2e-9
    engine.dft_clear()


# ---- 5. reference SCF runs ------------------------------------------------------------------------------------------------------

# Trajectories that depend on the eigensolver's choice, in the reference as well, so that only the first energy and the converged state
# compare (the converged energies agree to 2e-12 Eh on an MI355X):
#  * a degenerate pi pair AT the Fermi level of one spin in the first Fock matrices -- NO (alpha pi*^1), OH (beta pi^3), and O2 with a
#    pure local functional from the core guess (SVWN / STO-3G: iteration 3 already differs by 10 Eh, with either damping) -- takes an
#    arbitrary member of the pair; the quadrature grid is not invariant under every rotation about the axis, so the choice moves the
#    next energies (as test_gpu_dft.py shows for HF / 6-31G with a pure functional);
#  * homonuclear O2 with dynamic damping: the damping factor is rounding-noise driven in the reference (test_gpu_scf.py, UHF).
DEGENERATE_AT_FERMI = {"no_blyp_631g", "oh_b3lypg_ccpvdz", "o2_svwn_sto3g"}


@pytest.mark.parametrize("damping", [True, False])
@pytest.mark.parametrize("tag", TAGS)
def test_uks_scf_matches_reference(engine, uks, tag, damping):
    g = uks[tag]
    sfx = "" if damping else "_nodamp"
    atoms, shells, aos, na, nb, f, _ = _setup(engine, tag)
    xyz, chg = [a.origin for a in atoms], [float(a.charge) for a in atoms]
    S, T, V, _, _ = engine.one_electron(xyz, chg, [0, 0, 0.0])
    X, _, _ = engine.orthogonaliser(S)
    ranges = [sum(s.n_sph for s in shells if s.atom == a) for a in range(len(atoms))]
    r = engine.scf_uks(S, T, V, g["P0_alpha"], g["P0_beta"], float(g["E0"]), na, nb, mol.nuclear_repulsion(atoms), X=X, conv="extreme",
                       damping="dynamic" if damping else "none", hfx=f["hfx"], n_atom_ao=ranges, max_iter=int(g["max_iter"]))
    engine.dft_clear()
    ref = g["table" + sfx]
    n = min(r["n_iter"], len(ref))
    dE = abs(r["energy"] - float(g["energy" + sfx]))
    print(f"MEASURED scf {tag}{sfx}: dE {dE:.2e} iters {r['n_iter']} / {len(ref)}")
    assert dE < 1e-8
    np.testing.assert_allclose(r["components"][:5], g["components" + sfx], atol=1e-7)
    np.testing.assert_allclose(r["epsilons_spin"][0], g["eps_alpha" + sfx], atol=1e-6)
    np.testing.assert_allclose(r["epsilons_spin"][1], g["eps_beta" + sfx], atol=1e-6)
    assert abs(r["table"][0, 1] - ref[0, 1]) < 5e-8
    if tag in DEGENERATE_AT_FERMI or (damping and tag.startswith("o2")):
        return
    assert abs(r["n_iter"] - len(ref)) <= 1
    np.testing.assert_allclose(r["table"][:n, 1], ref[:n, 1], atol=5e-8)
    np.testing.assert_allclose(r["table"][:n, 6], ref[:n, 6], atol=1e-6)


# ---- 6. closed-shell singlet through the unrestricted cycle -----------------------------------------------------------------------

def test_singlet_through_uks_gives_rks(engine):
    """N2 / 6-31G, BLYP: scf_uks from P_alpha0 = P_beta0 = P0 / 2 stays on the restricted solution: the RKS energy to 1e-9."""
    from tuna_amd import dft
    from oracle import scf_oracle as so
    atoms = mol.make_atoms(["N", "N"], mol.angstrom_to_bohr(1.0977))
    shells = mol.build_shells(atoms, "6-31G")
    engine.set_basis(mol.expand_cartesian_aos(shells)).build_eri(True)
    pts, wts, _ = dft.integration_grid(atoms, "loose")
    f = engine.dft_setup(pts, wts, "BLYP")
    xyz, chg = [a.origin for a in atoms], [float(a.charge) for a in atoms]
    S, T, V, _, _ = engine.one_electron(xyz, chg, [0, 0, 0.0])
    X, _, _ = engine.orthogonaliser(S)
    P0, E0 = so.core_guess(T, V, X, 7)
    ranges = [sum(s.n_sph for s in shells if s.atom == a) for a in range(len(atoms))]
    V_NN = mol.nuclear_repulsion(atoms)
    rr = engine.scf_rhf(S, T, V, P0, E0, 7, V_NN, X=X, conv="extreme", hfx=f["hfx"], n_atom_ao=ranges)
    ru = engine.scf_uks(S, T, V, P0 / 2, P0 / 2, E0, 7, 7, V_NN, X=X, conv="extreme", hfx=f["hfx"], n_atom_ao=ranges)
    engine.dft_clear()
    print(f"MEASURED singlet: RKS {rr['energy']:.12f} UKS {ru['energy']:.12f} diff {abs(rr['energy'] - ru['energy']):.2e}")
    assert abs(rr["energy"] - ru["energy"]) < 1e-9


# ---- 7. input lines -------------------------------------------------------------------------------------------------------------

def test_input_lines(uks):
    from tuna_amd.energy import run
    gold = float(uks["o2_b3lyp_ccpvdz"]["energy"])
    lines = []
    out = run("SPE : O O 1.2075 : B3LYP CC-PVDZ : ML 3 EXTREME COREGUESS", silent=False, log=lines.append)
    print(f"MEASURED input line B3LYP ML 3: {abs(out.energy - gold):.2e}")
    assert abs(out.energy - gold) < 1e-8
    label = [s for s in lines if "energy:" in s and "Unrestricted" in s]
    assert label == ["\n Unrestricted B3LYP energy: " + " " * 3 + "    " + f"{out.energy:16.10f}"]    # tuna_kernel.py:856-858 spacing
    out2 = run("SPE : O O 1.2075 : UB3LYP CC-PVDZ : ML 3 EXTREME COREGUESS")
    assert abs(out2.energy - gold) < 1e-8
    out3 = run("SPE : H : B3LYP CC-PVDZ : ML 2")
    assert np.isfinite(out3.energy) and out3.energy < -0.49
    with pytest.raises(TunaError, match="singlet"):
        run("SPE : N N 1.0977 : UB3LYP CC-PVDZ")


# ---- 8. error paths and reproducibility -----------------------------------------------------------------------------------------

def test_error_paths_and_repeatability(engine, uks):
    g = uks["o2_b3lyp_sto3g"]
    atoms, shells, aos, na, nb, f, _ = _setup(engine, "o2_b3lyp_sto3g")
    rc1 = _vxcu_rc(engine, g["P0_alpha"], g["P0_beta"])
    rc2 = _vxcu_rc(engine, g["P0_alpha"], g["P0_beta"])
    assert rc1[0] == 0 and rc2[0] == 0
    assert np.array_equal(rc1[1], rc2[1]) and np.array_equal(rc1[2], rc2[2])
    assert np.array_equal(rc1[3], rc2[3]) and np.array_equal(rc1[4], rc2[4]) and rc1[5] == rc2[5]
    xyz, chg = [a.origin for a in atoms], [float(a.charge) for a in atoms]
    S, T, V, _, _ = engine.one_electron(xyz, chg, [0, 0, 0.0])
    V_NN = mol.nuclear_repulsion(atoms)
    # tf_scf_uhf with a grid set keeps refusing
    with pytest.raises(TunaError) as e:
        engine.scf_uhf(S, T, V, g["P0_alpha"], g["P0_beta"], float(g["E0"]), na, nb, V_NN)
    assert e.value.code == TF_EINVAL and "not implemented" in str(e.value)
    # tf_scf_uks without a grid
    engine.dft_clear()
    with pytest.raises(TunaError) as e:
        engine.scf_uks(S, T, V, g["P0_alpha"], g["P0_beta"], float(g["E0"]), na, nb, V_NN)
    assert e.value.code == TF_EINVAL and "tf_dft_setup" in str(e.value)
    rc = _vxcu_rc(engine, g["P0_alpha"], g["P0_beta"])[0]
    assert rc == TF_EINVAL
    # still usable: the same evaluation after a fresh setup gives the same bits
    _setup(engine, "o2_b3lyp_sto3g")
    rc3 = _vxcu_rc(engine, g["P0_alpha"], g["P0_beta"])
    assert rc3[0] == 0 and np.array_equal(rc3[1], rc1[1]) and np.array_equal(rc3[2], rc1[2])
    engine.dft_clear()


def test_sharded_context_refuses_uks(uks):
    """world > 1: tf_scf_uks returns TF_EINVAL before any collective; the context stays usable."""
    from tuna_amd.engine import Engine
    g = uks["o2_b3lyp_sto3g"]
    sym, R, basis, na, nb, method, grid = _spec("o2_b3lyp_sto3g")
    from tuna_amd import dft
    atoms = mol.make_atoms(sym, R)
    shells = mol.build_shells(atoms, basis)
    with Engine(0, 0, 2) as eng:                                   # rank 0 of 2
        eng.set_basis(mol.expand_cartesian_aos(shells)).build_eri(True)
        pts, wts, _ = dft.integration_grid(atoms, grid)
        eng.dft_setup(pts, wts, method)
        xyz, chg = [a.origin for a in atoms], [float(a.charge) for a in atoms]
        S, T, V, _, _ = eng.one_electron(xyz, chg, [0, 0, 0.0])
        with pytest.raises(TunaError) as e:
            eng.scf_uks(S, T, V, g["P0_alpha"], g["P0_beta"], float(g["E0"]), na, nb, mol.nuclear_repulsion(atoms))
        assert e.value.code == TF_EINVAL and "unsharded" in str(e.value)
        Va, Vb, n, ex, ec = eng.dft_vxc_unrestricted(g["P0_alpha"], g["P0_beta"])
        assert abs(n[0] + n[1] - 16.0) < 1e-2
