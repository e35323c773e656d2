"""CPU: the spin-polarised reference of tests/xc_reference_spin.py against mpmath, against the closed-shell reference at zeta = 0 and
against the reference program's own unrestricted V_XC of the guess densities (tests/golden/uks_systems.npz)."""
import os

import numpy as np
import pytest

import xc_reference as xr
import xc_reference_spin as xs
from tuna_amd import molecule as mol
from tuna_amd.spherical import transformation_matrix

PAIRS = [(x, c) for x in range(4) for c in range(6) if x or c]
# (rho_a, rho_b, sigma_aa, sigma_ab, sigma_bb): generic points, a negative sigma_ab, a weakly polarised one, large and small densities
POINTS = [(0.3, 0.1, 0.2, -0.05, 0.04), (0.8, 0.75, 1.1, 0.9, 0.8), (2.0, 0.5, 5.0, 1.0, 0.3), (1e4, 3e3, 1e9, 2e8, 5e7),
          (2e-6, 1e-6, 1e-13, 5e-14, 3e-14)]


@pytest.mark.parametrize("xid,cid", PAIRS)
def test_complex_step_agrees_with_mpmath(xid, cid):
    worst = 0.0
    for p in POINTS:
        fa, fb, fc, der = xs.point_derivs(xid, cid, 0.8, 1.0, *[[v] for v in p])
        cs = [0.8 * (fa[0] + fb[0]) + fc[0]] + [d[0] for d in der]
        mp = xs.mp_point(xid, cid, 0.8, 1.0, *p)
        scale = max(abs(v) for v in mp[1:3])
        for k, (a, b) in enumerate(zip(cs, mp)):
            err = abs(a - b) / max(abs(b), 1e-300 if k == 0 else scale * 1e-3)
            worst = max(worst, err)
            assert err < 1e-12, (xid, cid, p, k, a, b)
    print(f"MEASURED mpmath ({xid},{cid}): {worst:.2e}")


def test_complex_step_at_the_beta_floor():
    """rho_beta on the floor and just above it (zeta = 1 in double): every derivative against mpmath."""
    for p in ((0.5, 1e-23, 0.3, 0.0, 1e-46), (3e-4, 1e-23, 4e-7, 0.0, 1e-46), (0.5, 1e-15, 0.3, -1e-9, 1e-20)):
        for xid, cid in PAIRS:
            fa, fb, fc, der = xs.point_derivs(xid, cid, 0.8, 1.0, *[[v] for v in p])
            cs = [0.8 * (fa[0] + fb[0]) + fc[0]] + [d[0] for d in der]
            mp = xs.mp_point(xid, cid, 0.8, 1.0, *p)
            scale = max(abs(v) for v in mp[1:3])
            for k, (a, b) in enumerate(zip(cs, mp)):
                assert abs(a - b) <= 1e-12 * max(abs(b), 1e-300 if k == 0 else scale * 1e-3), (xid, cid, p, k, a, b)


def test_zeta_zero_is_the_closed_shell_reference():
    n = np.array([1e-8, 1e-3, 0.3, 5.0, 1e4])
    s = np.array([1e-20, 1e-7, 0.2, 3.0, 1e9])
    for cid in range(6):
        a = xs.f_c_spin(xs._NP, cid, n / 2, n / 2, s / 4, s / 4, s / 4)
        b = xr.f_c(xr._NP, cid, n, s)
        assert np.all(np.abs(a - b) <= 1e-14 * np.abs(b)), cid
    for xid in range(4):
        fa, fb = xs.f_x_spin(xs._NP, xid, n / 2, n / 2, s / 4, s / 4, 2.0 / 3.0)
        b = xr.f_x(xr._NP, xid, n, s, 2.0 / 3.0)
        assert np.all(np.abs(fa + fb - b) <= 1e-14 * np.abs(b)), xid


@pytest.fixture(scope="module")
def uks(golden):
    z = golden("uks_systems")
    out = {}
    for key in z.files:
        tag, name = key.split("__", 1)
        out.setdefault(tag, {})[name] = z[key]
    return out


def _systems():
    from conftest import GOLD
    g = np.load(os.path.join(GOLD, "uks_systems.npz"))
    tags = sorted({k.split("__", 1)[0] for k in g.files})
    out = {}
    for t in tags:
        R = float(g[t + "__R"])
        out[t] = ([str(x) for x in g[t + "__symbols"]], None if np.isnan(R) else R, str(g[t + "__basis"]), int(g[t + "__n_alpha"]),
                  int(g[t + "__n_beta"]), str(g[t + "__functional"]), str(g[t + "__grid"]))
    return out


@pytest.mark.parametrize("tag", list(_systems()))
def test_reproduces_reference_guess_vxc(uks, tag):
    from tuna_amd import dft
    sym, R, basis, na, nb, method, grid = _systems()[tag]
    g = uks[tag]
    atoms = mol.make_atoms(sym, R)
    shells = mol.build_shells(atoms, basis)
    aos = mol.expand_cartesian_aos(shells)
    pts, wts, _ = dft.integration_grid(atoms, grid)
    assert np.asarray(wts).size == int(g["n_points"])
    xn, cn, dfx, hfx, dfc = dft.FUNCTIONALS[method]
    U = transformation_matrix([s.L for s in shells])
    Va, Vb, n, ex, ec = xs.vxc_unrestricted(aos, pts, wts, g["P0_alpha"], g["P0_beta"], dft.X_ID[xn], dft.C_ID[cn], dfx, dfc, U=U)
    err = max(np.abs(Va - g["V_XC0_alpha"]).max(), np.abs(Vb - g["V_XC0_beta"]).max(), *np.abs(np.array(n) - g["n0"]),
              *np.abs(np.array(ex) - g["EX0"]), abs(ec - float(g["EC0"])))
    print(f"MEASURED reference guess {tag}: {err:.2e}")
    # H atom: rho_beta is on the floor everywhere and zeta rounds to 1, where the reference forms (1 - zeta)^(1/3) from a rounded zeta
    # (see xc_reference_spin); measured 2.5e-9 absolute, max|V_beta| = 0.12
    assert err < (1e-7 if tag == "h_b3lyp_ccpvdz" else 1e-11)
