"""CPU: the NumPy model of TD-DFT / TDA (tests/xc_kernel_reference.py) against the reference program's own numbers
(tests/golden/tddft_systems.npz, tools/make_golden_tddft.py), so that the conventions -- the factors of 2 of the point kernels, the
compound index order, where K enters A and B -- are fixed before any device code is compared with the model:
  * the point kernels at the reference's own densities: the 400 picked points of every system and the ladder from 1e-23 to 1e3;
  * K_XC singlet and triplet, all-electron and with a frozen orbital, on the whole grid rebuilt here (tuna_amd.dft.integration_grid and
    xc_reference.ao_on_points; the picked points pin that the rebuilt grid is the reference's, point for point);
  * every TDA and TD-DFT energy, |mu| and f from the STORED K through the model's assembly and the reference's route of solution.

Measured here: point kernels within 8 eps of the sum of the magnitudes of their terms; K within 1.6e-15 (1e-3 of its bound);
energies within 3.9e-14 Eh (TDA) and 9.6e-14 Eh (TD-DFT) for the singlets, the triplets bit for bit (with a pure functional the triplet
matrices are Delta + K_T, the stored K itself)."""
import numpy as np
import pytest

import cis_reference as cr
import xc_kernel_reference as xk
from test_cis_reference import CIS_TOL, MOMENT_TOL, cluster_sums

POINT_TOL = 64 * xk.EPS          # of the sum of the magnitudes of the closed form's terms: a few dozen operations, one rounding each
TDDFT_TOL = 1e-10                # Eh per state, the bar of CIS: both sides solve the same 2 dim non-symmetric problem with LAPACK


@pytest.fixture(scope="module")
def tddft_golden(golden):
    return xk.split(golden("tddft_systems"))


def test_golden_file_holds_the_systems(tddft_golden):
    assert set(tddft_golden) == set(xk.SYSTEMS) | {"ladder"}
    for tag, (sym, R, basis, nocc, functional, grid) in xk.SYSTEMS.items():
        g = tddft_golden[tag]
        N = len(g["eps"])
        assert int(g["n_occ"]) == nocc and str(g["functional"]) == functional and str(g["grid"]) == grid
        assert np.allclose(g["P"], 2 * g["C"][:, :nocc] @ g["C"][:, :nocc].T, atol=1e-12)
        for nf in xk.frozen_variants(g):
            dim = (nocc - nf) * (N - nocc)
            assert g[f"K_fc{nf}_singlet"].shape == g[f"K_fc{nf}_triplet"].shape == (dim, dim)
            for method in ("TDA", "TDDFT"):
                pre = f"{method}_fc{nf}_"
                assert pre + "unstable" not in g                                   # every stored Kohn-Sham solution is stable
                assert len(g[pre + "E_singlet"]) == len(g[pre + "E_triplet"]) == dim and len(g[pre + "energies"]) == 2 * dim
                assert np.all(np.diff(g[pre + "energies"]) >= 0) and np.all(g[pre + "osc"][g[pre + "labels"] == 1] == 0)
    dims = {tag: (int(g["n_occ"]) * (len(g["eps"]) - int(g["n_occ"]))) for tag, g in tddft_golden.items() if tag != "ladder"}
    assert dims == {"h2_lda_sto3g": 1, "lih_hfs_sto3g": 8, "lih_svwn3_sto3g": 8, "hf_svwn_631g": 30, "co_lda_631g": 77}
    assert set(tddft_golden["ladder"]) == {"HFS", "VWN5", "VWN3"}
    for table in tddft_golden["ladder"].values():
        assert table.shape == (4, 200) and table[0, 0] == 1e-23 and abs(table[0, -1] - 1e3) < 1e-9


@pytest.mark.parametrize("tag", list(xk.SYSTEMS))
def test_point_kernels_at_the_picked_points(tddft_golden, tag):
    g = tddft_golden[tag]
    pk = xk.point_kernels(g["rho_pick"], xk.SYSTEMS[tag][4])
    assert np.array_equal(pk["rho"], g["rho_pick"]) and g["rho_pick"].min() == xk.FLOOR       # floored points are among the picks
    for k, mk, gk in (("f_X", "mag_X", "fx_pick"), ("f_CS", "mag_CS", "fcs_pick"), ("f_CT", "mag_CT", "fct_pick")):
        d = np.abs(pk[k] - g[gk])
        print(f"\n[{tag} {k}] max |d| / mag = {np.max(d / np.maximum(pk[mk], 1e-300)) / xk.EPS:.1f} eps")
        assert np.all(d <= POINT_TOL * pk[mk])
    assert np.all(pk["f_X"] < 0)
    if xk.SYSTEMS[tag][4] == "HFS":
        assert not pk["f_CS"].any() and not pk["f_CT"].any()


@pytest.mark.parametrize("name,functional", [("HFS", "HFS"), ("VWN5", "SVWN"), ("VWN3", "SVWN3")])
def test_point_kernels_on_the_density_ladder(tddft_golden, name, functional):
    """1e-23 (the floor) to 1e3: at the top the terms of the VWN forms cancel to 1e-6 of their magnitudes (measured: mag / |f| up to
    3.9e6 for f_C^S of VWN5), which is why the bound is relative to the magnitudes and not to the value."""
    L = tddft_golden["ladder"][name]
    pk = xk.point_kernels(L[0], functional)
    rows = (("f_X", "mag_X", 1),) if name == "HFS" else (("f_CS", "mag_CS", 2), ("f_CT", "mag_CT", 3))
    for k, mk, row in rows:
        d = np.abs(pk[k] - L[row])
        print(f"\n[{name} {k}] max |d| / mag = {np.max(d / pk[mk]) / xk.EPS:.1f} eps, largest mag / |f| = {np.max(pk[mk] / np.abs(pk[k])):.1e}")
        assert np.all(d <= POINT_TOL * pk[mk]) and np.all(np.isfinite(pk[k]))
    if name != "HFS":
        assert np.max(pk["mag_CS"] / np.abs(pk["f_CS"])) > 1e5


@pytest.mark.parametrize("tag", list(xk.SYSTEMS))
def test_kernel_matrices_on_the_rebuilt_grid(tddft_golden, tag):
    """The rebuilt grid is the reference's (points bit for bit, weights to 4 ulp at the picks); the density on it agrees with the
    reference's within RHO_TOL of the sum of the magnitudes of its terms -- a failure of its own -- and K within
    2 gamma_G S + RHO_TOL D: two float64 sums of the same G terms in some order, plus what such a density difference can move."""
    g = tddft_golden[tag]
    r = xk.rebuilt(tag)
    pick = g["pick"]
    assert r["wts"].size == int(g["n_points"]) and np.array_equal(r["pts"][:, pick], g["pts_pick"])
    assert np.all(np.abs(r["wts"][pick] - g["w_pick"]) <= 4 * xk.EPS * np.abs(g["w_pick"]))
    for nf in xk.frozen_variants(g):
        m = xk.model_kernel(tag, g, nf)
        d_rho = np.abs(m["rho"][pick] - g["rho_pick"])
        assert np.all(d_rho <= xk.RHO_TOL * m["rho_mag"][pick]), (d_rho / m["rho_mag"][pick]).max()
        for mult, K, S, D in (("singlet", m["KS"], m["SS"], m["DS"]), ("triplet", m["KT"], m["ST"], m["DT"])):
            want = g[f"K_fc{nf}_{mult}"]
            bound = 2 * xk.gamma(m["G"]) * S + xk.RHO_TOL * D
            d = np.abs(K - want)
            print(f"\n[{tag} fc{nf} {mult}] dim {len(K)} G {m['G']} max |dK| {d.max():.1e} max |K| {np.abs(want).max():.3f} max |dK| / bound {np.max(d / bound):.1e} "
                  f"(largest bound {bound.max():.1e})")
            assert np.all(d <= bound) and bound.max() < 1e-9


@pytest.mark.parametrize("tag", list(xk.SYSTEMS))
def test_energies_from_the_stored_kernel(tddft_golden, tag):
    """The model's assembly with the STORED K and hfx of the functional, solved by eigh (TDA) and by the 2 dim eig (TD-DFT), against
    every stored energy; |mu| and f of the singlets as sums over clusters of degenerate states."""
    g = tddft_golden[tag]
    r = xk.rebuilt(tag)
    E = cr.dense_eri(r["aos"], r["shells"])
    nocc, hfx = int(g["n_occ"]), xk.FUNCTIONALS[xk.SYSTEMS[tag][4]][3]
    assert hfx == 0.0
    for nf in xk.frozen_variants(g):
        m = xk.matrices(E, g["C"], g["eps"], nocc, nf, hfx, g[f"K_fc{nf}_singlet"], g[f"K_fc{nf}_triplet"])
        assert np.abs(m["minus"] - np.diag(np.diag(m["minus"]))).max() < 1e-14        # pure functional: A - B = Delta
        for method, tda, tol in (("TDA", True, CIS_TOL), ("TDDFT", False, TDDFT_TOL)):
            pre = f"{method}_fc{nf}_"
            s = xk.solve(m, tda)
            d = [np.abs(s[f"E_{mult}"] - g[pre + f"E_{mult}"]).max() for mult in ("singlet", "triplet")]
            _, mag, f = cr.transition_moments(g["dip"], g["C"], nocc, nf, s["XpY_singlet"], s["E_singlet"])
            e, lab, mu, osc = cr.merged(s["E_singlet"], s["E_triplet"], mag, f)
            ge = g[pre + "energies"]
            d_mu = np.abs(cluster_sums(ge, mu) - cluster_sums(ge, g[pre + "tdm"])).max()
            d_f = np.abs(cluster_sums(ge, osc) - cluster_sums(ge, g[pre + "osc"])).max()
            print(f"\n[{tag} {method} fc{nf}] max |dE| singlet {d[0]:.1e} triplet {d[1]:.1e} cluster |mu| d {d_mu:.1e} f d {d_f:.1e}")
            assert max(d) < tol and np.abs(e - ge).max() < tol and d_mu < MOMENT_TOL and d_f < MOMENT_TOL
        # the Cholesky route of the library gives the reference's roots: what the GPU tests' TD-DFT bound rests on
        for mult in ("singlet", "triplet"):
            c = cr.tdhf_cholesky(m[f"plus_{mult}"], m["minus"])
            assert c["min_eig_minus"] > 0 and c["min_w2"] > 0
            assert np.abs(c["E"] - g[f"TDDFT_fc{nf}_E_{mult}"]).max() < TDDFT_TOL


def test_wrong_conventions_would_show(tddft_golden):
    """A kernel without its factor of 2, or the triplet weights in the singlet matrix, moves the energies far beyond the bound"""
    tag = "co_lda_631g"
    g = tddft_golden[tag]
    r = xk.rebuilt(tag)
    E = cr.dense_eri(r["aos"], r["shells"])
    KS, KT = g["K_fc0_singlet"], g["K_fc0_triplet"]
    for wrong in ((0.5 * KS, 0.5 * KT), (KT, KS)):
        s = xk.solve(xk.matrices(E, g["C"], g["eps"], 7, 0, 0.0, *wrong), True)
        assert np.abs(s["E_singlet"] - g["TDA_fc0_E_singlet"]).max() > 1e-3
