"""CPU: the NumPy model of the spin-resolved exchange-correlation kernel (tests/xc_kernel_spin_reference.py) against the reference
program's own numbers (tests/golden/utddft_systems.npz, written by tools/make_golden_utddft.py) -- the five point kernels on the ladder of
(rho_alpha, rho_beta) pairs and at the picked grid points, K of every stored system and window, every TDA and TD-DFT energy, |mu| and f
of the stable systems, the lowest Hessian eigenvalues, restricted and unrestricted -- and identities that hold without the reference:
at rho_alpha = rho_beta, f_aa + f_ab and f_aa - f_ab are the restricted singlet and triplet kernels of xc_kernel_reference.py; exchanging
alpha and beta exchanges f_aa and f_bb to the bit; and the kernels are the finite differences of the first derivatives that
xc_reference_spin.py takes by complex steps of the energy density.  The conditions the golden tool asserts are asserted again."""
import numpy as np
import pytest

import cis_reference as cr
import ucis_reference as ur
import xc_kernel_reference as xk
import xc_kernel_spin_reference as xs
import xc_reference_spin as xrs
from test_cis_reference import CIS_TOL, MOMENT_TOL, TDHF_TOL, cluster_sums
from test_ucis_reference import STAB_TOL
from xc_reference import C_VWN3, C_VWN5

POINT_ROWS = ("f_X_aa", "f_X_bb", "f_C_aa", "f_C_ab", "f_C_bb")


@pytest.fixture(scope="module")
def utddft_golden(golden):
    return xk.split(golden("utddft_systems"))


@pytest.fixture(scope="module")
def dense_eri():
    cache = {}

    def get(tag):
        if tag not in cache:
            _, shells, aos = xs.system(tag)
            cache[tag] = cr.dense_eri(aos, shells)
        return cache[tag]
    return get


def test_golden_conditions(utddft_golden):
    """what tools/make_golden_utddft.py asserts: the stored systems are those of the model's table, at least four are stable, between them
    they cover HFS, VWN3 and VWN5 and include one with o_beta <= 1; the size stays under the 450 KB of the golden tools"""
    import os
    from conftest import GOLD
    assert set(utddft_golden) - {"ladder", "rks"} == set(xs.SYSTEMS)
    ok = [t for t in xs.SYSTEMS if all(xs.stable(utddft_golden[t], k) for k in xs.frozen_variants(utddft_golden[t]))]
    assert len(ok) >= 4
    assert {xk.FUNCTIONALS[xs.SYSTEMS[t][5]][1] for t in ok} >= {None, "VWN3", "VWN5"}
    assert any(int(utddft_golden[t]["n_beta"]) <= 1 for t in ok) and any(int(utddft_golden[t]["n_beta"]) == 0 for t in ok)
    assert os.path.getsize(os.path.join(GOLD, "utddft_systems.npz")) <= 450 * 1024
    # the unstable systems carry the markers only, and a negative Hessian eigenvalue
    for t in xs.UNSTABLE:
        g = utddft_golden[t]
        assert t not in ok and all(f"{m}_fc{k}_unstable" in g and f"{m}_fc{k}_energies" not in g for m in ("TDA", "TDDFT") for k in xs.frozen_variants(g))
        assert all(float(g[f"stab_fc{k}_lowest"]) <= -1e-5 for k in xs.frozen_variants(g))
    assert all(float(utddft_golden[t]["stab_fc0_lowest"]) > 1e-6 for t in ok)
    for t in xs.SYSTEMS:
        g = utddft_golden[t]
        assert (int(g["n_alpha"]), int(g["n_beta"]), str(g["functional"])) == (xs.SYSTEMS[t][3], xs.SYSTEMS[t][4], xs.SYSTEMS[t][5])


@pytest.mark.parametrize("name,functional", [("HFS", "HFS"), ("VWN5", "SVWN"), ("VWN3", "SVWN3")])
def test_ladder(utddft_golden, name, functional):
    """the five kernels on the ladder -- zeta = 0, +-0.3, +-0.9, +-(1 - 1e-9), +-1 with the other spin exactly at the floor, both at the
    floor, a raw zero -- within POINT_TOL of the sums of the magnitudes of the model's terms; the floors are the reference's"""
    lad = utddft_golden["ladder"][name]
    pk = xs.point_kernels(lad[0], lad[1], functional)
    assert np.array_equal(pk["rho_a"], lad[0]) and np.array_equal(pk["rho_b"], lad[1]) and lad[:2].min() == xs.FLOOR
    for row, k in enumerate(POINT_ROWS, start=2):
        if (name == "HFS") != k.startswith("f_X"):
            assert not lad[row].any() or name != "HFS"
            continue
        d = np.abs(pk[k] - lad[row])
        assert np.isfinite(lad[row]).all()
        worst = np.max(d / np.maximum(pk["mag_" + k], 1e-300)) / xs.EPS
        print(f"\n[{name} {k}] max |model - reference| / mag = {worst:.2f} eps over {lad.shape[1]} pairs")
        assert np.all(d <= xs.POINT_TOL * pk["mag_" + k])


@pytest.mark.parametrize("tag", list(xs.SYSTEMS))
def test_picked_points(utddft_golden, tag):
    """at the 400 picked points of every system: the model's densities on the rebuilt grid against the reference's within RHO_TOL of the
    sums of the magnitudes of their terms, and the five kernels at the reference's densities within POINT_TOL of theirs"""
    g, r = utddft_golden[tag], xs.rebuilt(tag)
    pick = g["pick"]
    assert len(r["wts"]) == int(g["n_points"]) and np.allclose(r["pts"][:, pick], g["pts_pick"], rtol=0, atol=1e-12)
    for s, P in (("a", g["P_alpha"]), ("b", g["P_beta"])):
        rho, mag = xk.density(r["phi"][pick], P)
        assert np.all(np.abs(np.maximum(rho, xs.FLOOR) - g[f"rho_{s}_pick"]) <= xk.RHO_TOL * mag + 1e-300)
    pk = xs.point_kernels(g["rho_a_pick"], g["rho_b_pick"], xs.SYSTEMS[tag][5])
    for k, key in zip(POINT_ROWS, ("fxaa_pick", "fxbb_pick", "fcaa_pick", "fcab_pick", "fcbb_pick")):
        assert np.all(np.abs(pk[k] - g[key]) <= xs.POINT_TOL * pk["mag_" + k]), k


@pytest.mark.parametrize("tag", list(xs.SYSTEMS))
def test_kernel_matrix_and_states(utddft_golden, dense_eri, tag):
    """K of every window within the model's bound (k_bound); then, for the stable systems, every TDA and TD-DFT energy and the cluster
    sums of |mu| and f from the model's matrices (hfx = 0: A = Delta + G + K, B = G + K), and the lowest Hessian eigenvalue.  Allowed:
    the bounds of test_cis_reference.py plus the Frobenius norm of the bound of K (an eigenvalue of a symmetric matrix moves by no
    more than the norm of the perturbation)."""
    g = utddft_golden[tag]
    E = dense_eri(tag)
    na, nb = int(g["n_alpha"]), int(g["n_beta"])
    Ca, Cb, ea, eb = g["C_alpha"], g["C_beta"], g["eps_alpha"], g["eps_beta"]
    for k in xs.frozen_variants(g):
        m = xs.golden_model(tag, g, k)
        bound = xs.k_bound(m)
        d = np.abs(m["K"] - g[f"K_fc{k}"])
        dK = np.linalg.norm(bound)
        print(f"\n[{tag} fc{k}] dim {len(d)} max |dK| {d.max():.1e} max |dK| / bound {np.max(d / np.maximum(bound, 1e-300)):.1e} ||bound|| {dK:.1e}")
        assert np.all(d <= bound)
        mats = xs.matrices(E, Ca, Cb, ea, eb, na, nb, k // 2, k // 2, 0.0, m["K"])
        spectra, lowest = ur.hessian_spectra_uhf(mats)
        assert abs(lowest - float(g[f"stab_fc{k}_lowest"])) <= STAB_TOL + 2 * dK
        if not xs.stable(g, k):
            continue
        for method, base in (("TDA", CIS_TOL), ("TDDFT", TDHF_TOL)):
            pre = f"{method}_fc{k}_"
            if method == "TDA":
                e, V = ur.cis(mats["A"])
            else:
                e, X, Y = ur.tdhf_full(mats["A"], mats["B"])
                V = X + Y
            ge = g[pre + "energies"]
            assert len(e) == len(ge) == mats["A"].shape[0]                                 # no state is left out
            mu3, mu, f = ur.transition_moments(g["dip"], Ca, Cb, na, nb, k // 2, k // 2, V, e)
            d_e = np.abs(e - ge).max()
            d_mu = np.abs(cluster_sums(ge, mu) - cluster_sums(ge, g[pre + "tdm"])).max()
            d_f = np.abs(cluster_sums(ge, f) - cluster_sums(ge, g[pre + "osc"])).max()
            print(f"[{tag} {method} fc{k}] max |dE| {d_e:.1e} (tol {base + dK:.1e}) cluster |mu| d {d_mu:.1e} f d {d_f:.1e}")
            assert d_e <= base + dK and d_mu <= MOMENT_TOL and d_f <= MOMENT_TOL


@pytest.mark.parametrize("tag", list(xk.SYSTEMS))
def test_restricted_kohn_sham_stability(golden, utddft_golden, tag):
    """rks__<tag>__singlet / triplet: the lowest eigenvalues of the restricted Kohn-Sham Hessians of the systems of tddft_systems.npz from
    the restricted model's matrices (xc_kernel_reference.matrices with its K_S, K_T)"""
    g = xk.split(golden("tddft_systems"))[tag]
    _, shells, aos = xk.system(tag)
    E = cr.dense_eri(aos, shells)
    m = xk.model_kernel(tag, g, 0)
    hfx = xk.FUNCTIONALS[xk.SYSTEMS[tag][4]][3]
    mats = xk.matrices(E, g["C"], g["eps"], int(g["n_occ"]), 0, hfx, m["KS"], m["KT"])
    g2 = 2 * xk.gamma(m["G"])
    dK = np.linalg.norm(g2 * m["SS"] + xk.RHO_TOL * m["DS"]) + np.linalg.norm(g2 * m["ST"] + xk.RHO_TOL * m["DT"])
    low = {mult: min(np.linalg.eigvalsh(mats[f"plus_{mult}"])[0], np.linalg.eigvalsh(mats["minus"])[0]) for mult in ("singlet", "triplet")}
    for mult in ("singlet", "triplet"):
        want = float(utddft_golden["rks"][f"{tag}__{mult}"])
        print(f"\n[{tag} {mult}] lowest {low[mult]:.10f} golden {want:.10f}")
        assert abs(low[mult] - want) <= STAB_TOL + 2 * dK


# ---- identities that hold without the reference ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("functional", ["HFS", "SVWN", "SVWN3"])
def test_equal_spin_densities_give_the_restricted_kernels(functional):
    n = np.logspace(-22, 3, 300)
    pk, pr = xs.point_kernels(n / 2, n / 2, functional), xk.point_kernels(n, functional)
    mag = pk["mag_f_X_aa"] + pk["mag_f_C_aa"] + pk["mag_f_C_ab"] + pr["mag_X"]
    assert np.all(np.abs(pk["f_X_aa"] + pk["f_C_aa"] + pk["f_C_ab"] - pr["f_X"] - pr["f_CS"]) <= xs.POINT_TOL * (mag + pr["mag_CS"]))
    assert np.all(np.abs(pk["f_X_aa"] + pk["f_C_aa"] - pk["f_C_ab"] - pr["f_X"] - pr["f_CT"]) <= xs.POINT_TOL * (mag + pr["mag_CT"]))
    assert np.array_equal(pk["f_C_aa"], pk["f_C_bb"]) and np.array_equal(pk["f_X_aa"], pk["f_X_bb"])


@pytest.mark.parametrize("functional", ["HFS", "SVWN", "SVWN3"])
def test_exchanging_the_spins_exchanges_the_kernels(functional):
    rng = np.random.default_rng(3)
    ra, rb = 10.0 ** rng.uniform(-22, 2, 500), 10.0 ** rng.uniform(-22, 2, 500)
    p, q = xs.point_kernels(ra, rb, functional), xs.point_kernels(rb, ra, functional)
    for a, b in (("f_X_aa", "f_X_bb"), ("f_C_aa", "f_C_bb"), ("f_C_ab", "f_C_ab"), ("f_C_bb", "f_C_aa")):
        assert np.array_equal(p[a], q[b]), (a, b)


@pytest.mark.parametrize("functional,cid", [("SVWN", C_VWN5), ("SVWN3", C_VWN3), ("HFS", 0)])
def test_kernels_are_derivatives_of_the_first_derivatives(functional, cid):
    """d (dF / d rho_s) / d rho_t by central differences of xc_reference_spin.point_derivs (complex steps of the energy density: no
    hand-derived formula) at two step sizes: D(h) - D(h / 2) is three times the error of D(h / 2), and the rounding of the quotient
    is 16 eps |v| / (h rho).  The model must agree within that.  A kernel with a wrong factor of 2 misses by itself."""
    xid, dfx, dfc = 1, 1.0, (0.0 if cid == 0 else 1.0)
    n = np.logspace(-3, 1, 9)
    for z in (0.0, 0.3, -0.3, 0.9, -0.9):
        ra, rb = n * (1 + z) / 2, n * (1 - z) / 2
        pk = xs.point_kernels(ra, rb, functional)
        want = {("a", "a"): pk["f_X_aa"] * dfx + dfc * pk["f_C_aa"], ("a", "b"): dfc * pk["f_C_ab"], ("b", "a"): dfc * pk["f_C_ab"],
                ("b", "b"): pk["f_X_bb"] * dfx + dfc * pk["f_C_bb"]}
        zero = np.zeros_like(ra)

        def first(xa, xb):
            return xrs.point_derivs(xid, cid, dfx, dfc, xa, xb, zero + 1e-46, zero, zero + 1e-46)[3][:2]

        def quotient(h, t):
            fa, fb = ((1 + h, 1 - h), (1, 1)) if t == "a" else ((1, 1), (1 + h, 1 - h))
            up, dn = first(ra * fa[0], rb * fb[0]), first(ra * fa[1], rb * fb[1])
            step = 2 * h * (ra if t == "a" else rb)
            return [(u - d) / step for u, d in zip(up, dn)], step
        for t in "ab":
            (coarse, _), (fine, step) = quotient(2e-4, t), quotient(1e-4, t)
            v = first(ra, rb)
            for si, s in enumerate("ab"):
                tol = np.abs(coarse[si] - fine[si]) + 16 * xs.EPS * np.abs(v[si]) / step * 2
                d = np.abs(fine[si] - want[(s, t)])
                assert np.all(d <= tol), (functional, z, s, t, (d / tol).max())
                assert np.all(tol < 1e-4 * np.abs(want[(s, t)])) or cid == 0 and s != t
                if not (cid == 0 and s != t):
                    assert np.all(np.abs(fine[si] - 2 * want[(s, t)]) > 100 * tol)
