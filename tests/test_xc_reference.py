"""CPU: the independent V_XC reference of tests/xc_reference.py checked on its own -- its complex-step functional derivatives
against mpmath at 40 digits, its AOs against the oracle's overlap matrix by quadrature on an extreme grid, and its V_XC, n_el,
E_X and E_C of the guess densities against the reference program's goldens.  tests/test_gpu_dft_reference.py then judges the
library by it."""
import numpy as np
import pytest

import xc_reference as xr
from conftest import DFT_SYSTEMS, R_N2
from tuna_amd import molecule as mol
from tuna_amd.spherical import transformation_matrix

PAIRS = [(x, c) for x in range(4) for c in range(6) if x or c]
N_SWEEP = [1e-20, 1e-17, 1e-14, 1e-12, 1e-10, 1e-7, 1e-4, 1e-2, 1.0, 1e2, 1e4, 1e6]
S_SWEEP = [0.0, 1e-30, 1e-12, 1e-4, 1.0, 1e4, 1e8]


def functional_ids(name):
    from tuna_amd import dft
    xn, cn, dfx, hfx, dfc = dft.FUNCTIONALS[name]
    return dft.X_ID[xn], dft.C_ID[cn], dfx, dfc


@pytest.mark.parametrize("xid,cid", PAIRS)
def test_complex_step_matches_mpmath(xid, cid):
    """df/dn and df/dsigma by complex step against mp.diff at 40 digits (and f itself), every kernel branch pair, sigma floored.
    Measured worst relative error: 2e-14 for n >= 1e-12.  Below that, VWN's own formula cancels in double precision: its log terms
    nearly cancel at large r_s (2e-10 of e at n = 1e-23, 4e-11 at n = 1e-20).  The kernel evaluates the same formula in double, so
    this is a property of the formula and not of the derivative.  Where the exact value is below 1e-200 (the LYP sigma derivative
    at n = 1e-10, about 1e-224), only an absolute comparison is meaningful."""
    for xa in (2.0 / 3.0, 0.7):
        for n in N_SWEEP:
            rtol = 1e-13 if n >= 1e-12 else 1e-9
            for s in S_SWEEP:
                n_f, s_f = xr.floors(np.array([n]), np.array([s]))
                got = np.array(xr.point_derivs(xid, cid, n_f, s_f, xa)).ravel()
                ref = np.array(xr.mp_point(xid, cid, n_f[0], s_f[0], xa))
                assert np.all(np.abs(got - ref) <= rtol * np.abs(ref) + 1e-200), (xid, cid, xa, n, s, got, ref)


def _n2(basis):
    atoms = mol.make_atoms(["N", "N"], R_N2)
    shells = mol.build_shells(atoms, basis)
    return atoms, shells, mol.expand_cartesian_aos(shells)


@pytest.mark.parametrize("basis,spherical", [("cc-pVQZ", True), ("6-31G*", False)])
def test_ao_overlap_by_quadrature(basis, spherical):
    """sum_g w phi_i phi_j on the extreme grid against the oracle's analytic overlap S, and n_el = tr(P S) for the core guess.
    The closed-form normalisation, the g-shell powers and the spherical map are all in this.  Measured on the extreme grid:
    |S_grid - S| <= 2.7e-14 (cc-pVQZ, spherical) and 1.0e-14 (6-31G*, Cartesian d); |tr(P S_grid) - tr(P S)| <= 1.3e-13.
    On the medium grid the same numbers are 1.8e-7 and 3.9e-9: the bars below hold only for the extreme grid."""
    from oracle import oracle, scf_oracle as so
    from tuna_amd import dft
    atoms, shells, aos = _n2(basis)
    S, T, V, _, _ = oracle.one_electron(aos, [a.origin for a in atoms], [7.0, 7.0], [0.0, 0.0, 0.0])
    U = transformation_matrix([s.L for s in shells]) if spherical else None
    if spherical:
        S, T, V = (so.to_spherical(U, M) for M in (S, T, V))
    pts, wts, _ = dft.integration_grid(atoms, "extreme")
    Sg = xr.overlap_on_grid(aos, pts, wts, U)
    assert np.abs(Sg - S).max() < 3e-13
    X, _, _ = so.orthogonaliser(S)
    P, _ = so.core_guess(T, V, X, 7)
    assert abs(np.sum(P * Sg) - 14.0) < 2e-12 and abs(np.sum(P * S) - 14.0) < 1e-12


@pytest.mark.parametrize("tag", list(DFT_SYSTEMS))
def test_reference_reproduces_the_goldens(dft_golden, tag):
    """V_XC, n_el, E_X and E_C of the guess density against the reference program's values, at the GPU tests' 1e-9 bars.
    Measured worst: 4.4e-14 in V, 5.3e-15 in E_X, 3.6e-15 in n_el."""
    from tuna_amd import dft
    g = dft_golden[tag]
    sym, R, basis, nocc, method, grid = DFT_SYSTEMS[tag]
    atoms = mol.make_atoms(sym, R)
    shells = mol.build_shells(atoms, basis)
    pts, wts, _ = dft.integration_grid(atoms, grid)
    xid, cid, dfx, dfc = functional_ids(method)
    V, n_el, ex, ec = xr.vxc(mol.expand_cartesian_aos(shells), pts, wts, g["P0"], xid, cid, dfx, dfc,
                             U=transformation_matrix([s.L for s in shells]))
    assert abs(n_el - float(g["n_el0"])) < 1e-9
    assert abs(ex - float(g["EX0"])) < 1e-9 and abs(ec - float(g["EC0"])) < 1e-9
    assert np.abs(V - g["V_XC0"]).max() < 1e-9
