"""GPU: tf_dft_setup / tf_dft_vxc (tuna_amd/csrc/tf_dft.hip.h) against the independent CPU reference of tests/xc_reference.py, at the
edges the goldens of test_gpu_dft.py never reach: single points from the density floor to 1e6 for every functional pair, g and h shells,
Cartesian d and f, converged / random / indefinite / non-symmetric densities, every split-K branch of the V GEMM, the lane edges of the
density kernel, V as the derivative of E_XC, a converged KS state without a golden, bitwise reproducibility and the error paths.

Every bar is about ten times the worst error measured on an MI355X; the measurements are in the docstrings."""
import ctypes

import numpy as np
import pytest

import xc_reference as xr
from conftest import R_AR2, R_CO, R_N2
from tuna_amd import molecule as mol
from tuna_amd._lib import ptr
from tuna_amd.spherical import transformation_matrix

pytestmark = pytest.mark.gpu

TF_EINVAL = -1
PAIRS = [(x, c) for x in range(4) for c in range(6) if x or c]
TOL_V, TOL_E = 2e-14, 5e-12                 # whole grids: ten times the worst measured (V relative to max|V|; integrals relative)


def _ids(name):
    from tuna_amd import dft
    xn, cn, dfx, hfx, dfc = dft.FUNCTIONALS[name]
    return dft.X_ID[xn], dft.C_ID[cn], dfx, dfc, hfx


def _raw_setup(engine, pts, wts, xid, cid, dfx=1.0, dfc=1.0, x_alpha=2.0 / 3.0):
    pts = np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(3, -1))
    wts = np.ascontiguousarray(np.asarray(wts, dtype=np.float64).reshape(-1))
    return engine._L.tf_dft_setup(engine._ctx, wts.size, ptr(pts), ptr(wts), xid, cid, float(dfx), float(dfc), float(x_alpha))


def _vxc_rc(engine, P):
    P = np.ascontiguousarray(P, dtype=np.float64)
    V = np.zeros_like(P)
    n, ex, ec = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    rc = engine._L.tf_dft_vxc(engine._ctx, ptr(P), ptr(V), ctypes.byref(n), ctypes.byref(ex), ctypes.byref(ec))
    return rc, V, n.value, ex.value, ec.value


class System:
    """A basis on the device (tf_build_eri in the requested representation), its reference AO map and a grid."""

    def __init__(self, engine, sym, R, basis, spherical=True, grid="loose"):
        from tuna_amd import dft
        self.atoms = mol.make_atoms(sym, R)
        self.shells = mol.build_shells(self.atoms, basis)
        self.aos = mol.expand_cartesian_aos(self.shells)
        engine.set_basis(self.aos).build_eri(spherical)
        self.U = transformation_matrix([s.L for s in self.shells]) if spherical else None
        self.N = engine.N
        self.pts, self.wts, _ = dft.integration_grid(self.atoms, grid) if isinstance(grid, str) else grid
        self.pts = np.asarray(self.pts).reshape(3, -1)
        self.wts = np.asarray(self.wts).reshape(-1)
        self._grid = None

    def ao_grid(self):
        if self._grid is None:
            self._grid = xr.ao_grid(self.aos, self.pts, self.U)
        return self._grid

    def ref(self, P, xid, cid, dfx, dfc, x_alpha=2.0 / 3.0):
        return xr.vxc(self.aos, self.pts, self.wts, P, xid, cid, dfx, dfc, x_alpha, grid=self.ao_grid())


def _compare(engine, sysm, P, name, tol_V, tol_E, label=""):
    xid, cid, dfx, dfc, _ = _ids(name)
    assert _raw_setup(engine, sysm.pts, sysm.wts, xid, cid, dfx, dfc) == 0, engine._L.tf_last_error(engine._ctx)
    rc, V, n_el, ex, ec = _vxc_rc(engine, P)
    assert rc == 0
    Vr, nr, exr, ecr = sysm.ref(P, xid, cid, dfx, dfc)
    eV = np.abs(V - Vr).max() / np.abs(Vr).max()
    eE = [abs(a - b) / abs(b) for a, b in ((n_el, nr), (ex, exr), (ec, ecr)) if b != 0.0]
    print(f"MEASURED {label} {name}: V {eV:.2e} E {max(eE):.2e}")
    assert eV < tol_V, (label, name, eV)
    assert max(eE) < tol_E, (label, name, eE)
    assert np.abs(V - V.T).max() == 0.0
    return V, n_el, ex, ec


# ---- per-point extremes ------------------------------------------------------------------------------------------------------

SP_BASIS = {7: [("S", [(0.9, 1.0)]), ("P", [(0.6, 1.0)])]}
RHO_SCALES = [1e-30, 1e-26, 1e-23, 1e-20, 1e-16, 1e-12, 1e-8, 1e-4, 1e-2, 1.0, 1e2, 1e4, 1e6]


def _single_point_cases(phi, coupled):
    """Density matrices on the s / p_z block that give rho from 1e-30 to 1e6 at the point, one indefinite one (raw rho < 0).
    Without the s-p_z coupling the density gradient at the nucleus is exactly zero."""
    P0 = np.zeros((4, 4))
    P0[0, 0], P0[3, 3] = 1.0, 0.5
    if coupled:
        P0[0, 3] = P0[3, 0] = 0.3
    rho0 = phi @ P0 @ phi
    out = [P0 * (s / rho0) for s in RHO_SCALES]
    Pn = np.zeros((4, 4))
    Pn[0, 0], Pn[3, 3] = -1.0, 0.2                                  # indefinite: raw rho < 0 at the point, floored to 1e-23
    out.append(Pn)
    return out


def test_single_point_extremes_every_functional(engine):
    """G = 1 on one N atom with one s and one p shell, the point on the z axis (off the nucleus: all of the s / p_z block of V is
    non-zero, and its three entries weigh v_rho and v_sigma differently) and at the nucleus (grad rho = 0 exactly, sigma floored).
    rho is swept from 1e-30 to 1e6, plus a negative raw rho; every functional id pair and Slater at x_alpha 2/3 and 0.7.  Reference:
    mpmath at 40 digits on the reference's own AO values.  Each V entry is compared relative to the sum of the magnitudes of its
    v_rho and v_sigma terms; n_el, E_X and E_C relative to themselves.
    Measured worst relative errors: 1.0e-14 without VWN; 2.3e-14 with VWN for rho >= 1e-12; 4.3e-10 with VWN below (VWN's own log
    terms cancel in double precision at large r_s: the NumPy form of the same formula differs from mpmath by as much,
    test_xc_reference.py).  Bars: 1e-13, 2e-13 and 1e-9 (the golden bar; the cancellation is deterministic)."""
    atoms = mol.make_atoms(["N"], None)
    aos = mol.expand_cartesian_aos(mol.build_shells(atoms, SP_BASIS))
    engine.set_basis(aos).build_eri(True)
    assert engine.N == 4
    worst = {}
    for z in (0.7, 0.0):
        pt = np.array([[0.0], [0.0], [z]])
        w = np.array([0.37])
        phi, dphi = xr.ao_on_points(aos, pt)
        phi, dphi = phi[0], dphi[:, 0, :]
        for xid, cid in PAIRS:
            for xa in ((2.0 / 3.0, 0.7) if xid else (2.0 / 3.0,)):
                assert _raw_setup(engine, pt, w, xid, cid, 1.0, 1.0, xa) == 0
                gga = xid >= 2 or cid >= 3
                for P in _single_point_cases(phi, z != 0.0):
                    rc, V, n_el, ex, ec = _vxc_rc(engine, P)
                    assert rc == 0
                    rho = phi @ P @ phi
                    g = 2.0 * dphi @ (P.T @ phi) if gga else np.zeros(3)     # 2 sum_ij P_ij phi_i grad phi_j
                    rho_f, sig_f = xr.floors(np.array([rho]), np.array([g @ g]))
                    fx, fc, xn, xs, cn, cs = xr.mp_point(xid, cid, rho_f[0], sig_f[0], xa)
                    vr, vs = xn + cn, xs + cs
                    gd = g @ dphi                                            # grad rho . grad phi_j
                    t_r = vr * np.outer(phi, phi)
                    t_s = 2.0 * vs * (np.outer(phi, gd) + np.outer(gd, phi)) if gga else 0.0 * t_r
                    Vr = w[0] * (t_r + t_s)
                    scale = w[0] * (np.abs(t_r) + np.abs(t_s))
                    mask = scale > 0
                    e = np.zeros(4)
                    e[0] = (np.abs(V - Vr)[mask] / scale[mask]).max() if mask.any() else np.abs(V).max()
                    assert np.abs(V[~mask]).max(initial=0.0) == 0.0
                    for k, (a, b) in enumerate(((n_el, w[0] * rho_f[0]), (ex, w[0] * fx), (ec, w[0] * fc))):
                        e[k + 1] = abs(a - b) / abs(b) if b != 0.0 else abs(a)
                    key = (xid, cid, "floor" if rho < 1e-23 else ("low" if rho < 1e-12 else "bulk"))
                    worst[key] = np.maximum(worst.get(key, np.zeros(4)), e)
    for key, e in sorted(worst.items()):
        print("MEASURED point", key, np.array2string(e, precision=1))
    for (xid, cid, band), e in worst.items():
        vwn = cid in (1, 2, 4, 5)                                     # VWN's formula cancels in double at tiny rho (test_xc_reference)
        bar = (1e-9 if band != "bulk" else 2e-13) if vwn else 1e-13
        assert e.max() < bar, ((xid, cid, band), e)


# ---- whole grids at densities that are not guesses ---------------------------------------------------------------------------

def _random_densities(N, rng, nocc):
    A = rng.standard_normal((N, nocc))
    P_psd = 2.0 * A @ A.T / N
    B = rng.standard_normal((N, N)) / N
    P_ind = P_psd + 0.5 * (B + B.T)
    P_ind = P_ind - 2.0 * np.abs(np.linalg.eigvalsh(P_ind)).max() * 0.05 * np.eye(N)
    assert N == 1 or np.linalg.eigvalsh(P_ind).min() < 0 < np.linalg.eigvalsh(P_ind).max()
    P_ns = P_psd + 0.3 * B                                         # non-symmetric: pins the operand order of grad rho
    return {"psd": P_psd, "indefinite": P_ind, "nonsym": P_ns}


def _converged(engine, sysm, nocc, name, grid_pts=None):
    from oracle import scf_oracle as so
    from tuna_amd import dft
    f = engine.dft_setup(sysm.pts, sysm.wts, name)
    xyz, chg = [a.origin for a in sysm.atoms], [float(a.charge) for a in sysm.atoms]
    S, T, V, _, _ = engine.one_electron(xyz, chg, [0, 0, 0.0], spherical=sysm.U is not None)
    X, _, _ = engine.orthogonaliser(S)
    P0, E0 = so.core_guess(T, V, X, nocc)
    r = engine.scf_rhf(S, T, V, P0, E0, nocc, mol.nuclear_repulsion(sysm.atoms), X=X, conv="tight", damping="dynamic", hfx=f["hfx"])
    engine.dft_clear()
    return r, S, T, V, X


WHOLE = {
    "ar2_ccpvqz": (["AR", "AR"], R_AR2, "cc-pVQZ", True, 18),
    "n2_ccpvqz": (["N", "N"], R_N2, "cc-pVQZ", True, 7),
    "n2_ccpv5z": (["N", "N"], R_N2, "cc-pV5Z", True, 7),
    "co_def2tzvp_cart": (["C", "O"], R_CO, "def2-TZVP", False, 7),
    "n2_631gstar_cart": (["N", "N"], R_N2, "6-31G*", False, 7),
}


@pytest.mark.parametrize("tag", list(WHOLE))
def test_whole_grid_vxc_at_converged_and_random_densities(engine, tag):
    """V_XC, n_el, E_X, E_C on loose grids for g (cc-pVQZ), h (cc-pV5Z) and Cartesian d / f shells: the converged B3LYP density
    against B3LYP, BLYP, SVWN3 and HFB (one per kernel branch), a random PSD, an indefinite and a non-symmetric P against the GGA
    branches.  V relative to max|V|, the integrals relative to themselves.  Measured worst: V 2.1e-15, n_el / E_X / E_C 4.5e-13
    (E_C of the indefinite P on cc-pV5Z, where floored points make it small); 1e-15 elsewhere."""
    sym, R, basis, spherical, nocc = WHOLE[tag]
    s = System(engine, sym, R, basis, spherical, "loose")
    r, *_ = _converged(engine, s, nocc, "B3LYP")
    Pc = r["P"]
    for name in ("B3LYP", "BLYP", "SVWN3", "HFB"):
        _compare(engine, s, Pc, name, TOL_V, TOL_E, f"{tag} converged")
    rng = np.random.default_rng(7)
    for kind, P in _random_densities(s.N, rng, nocc).items():
        _compare(engine, s, P, "B3LYP", TOL_V, TOL_E, f"{tag} {kind}")
    engine.dft_clear()


# ---- shape edges ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 127, 128, 129, 256, 128 * 100, 128 * 100 + 1, 128 * 173 + 77])
def test_split_k_branches(engine, G):
    """Real grid points and weights of CO / def2-TZVP (medium grid) subsampled to G points: G < 128 runs only the remainder GEMM,
    a multiple of 128 no remainder GEMM, the others both; B3LYP at a random PSD P.  The points are drawn from where the weight and
    the AOs matter and kept in random order, so that the remainder rows are as significant as the others (a real grid ends in the
    outer shell of atom B, where a shifted remainder operand changes nothing).  Measured worst: V 9.9e-16, integrals 5.3e-16."""
    from tuna_amd import dft
    atoms = mol.make_atoms(["C", "O"], R_CO)
    pts, wts, _ = dft.integration_grid(atoms, "medium")
    pts, wts = pts.reshape(3, -1), wts.reshape(-1)
    r = np.sqrt(pts[0] ** 2 + pts[1] ** 2 + (pts[2] - 0.5 * R_CO) ** 2)
    pool = np.flatnonzero((wts > 1e-6) & (r < 4.0))
    idx = np.random.default_rng(G).permutation(pool)[:G]
    assert idx.size == G
    s = System(engine, ["C", "O"], R_CO, "def2-TZVP", True, (pts[:, idx], wts[idx], None))
    P = _random_densities(s.N, np.random.default_rng(1), 7)["psd"]
    _compare(engine, s, P, "B3LYP", TOL_V, TOL_E, f"G={G}")
    engine.dft_clear()


def _one_atom_basis(N):
    if N == 1:
        return ["H"], "STO-3G"
    counts = {15: (3, 4, 0, 0), 16: (4, 4, 0, 0), 17: (2, 0, 3, 0)}[N]
    return ["N"], {7: mol.even_tempered_basis(*counts)}


@pytest.mark.parametrize("N", [1, 15, 16, 17])
def test_density_kernel_lane_edges(engine, N):
    """N of 1, 15, 16 and 17: the sixteen lanes per point of xc_density_kernel with fewer, as many and one more AO than lanes.
    Measured worst: V 2.3e-15, integrals 3.8e-14."""
    sym, basis = _one_atom_basis(N)
    s = System(engine, sym, None, basis, True, "loose")
    assert s.N == N
    P = _random_densities(N, np.random.default_rng(N), 1)["nonsym"]
    for name in ("B3LYP", "SVWN"):
        _compare(engine, s, P, name, TOL_V, TOL_E, f"N={N}")
    engine.dft_clear()


# ---- V is the derivative of E_XC ------------------------------------------------------------------------------------------------

_CONVERGED = {}


@pytest.mark.parametrize("name", ["B3LYP", "BLYP", "SVWN3", "HFB", "SLYP"])
def test_vxc_is_the_gradient_of_exc(engine, name):
    """(E_xc(P + h D) - E_xc(P - h D)) / 2h against <V_XC(P), D> for a random symmetric D at the converged CO / def2-TZVP density:
    GPU calls only, no reference formula.  A wrong factor on v_sigma or a wrong grad phi component breaks it.  Measured relative
    differences: 7e-7, 7e-9 and 1.7e-10 at h = 1e-3, 1e-4 and 1e-5 (truncation falls as h^2 down to rounding); bar 2e-9 at h = 1e-5."""
    s = System(engine, ["C", "O"], R_CO, "def2-TZVP", True, "loose")
    if "co" not in _CONVERGED:
        _CONVERGED["co"] = _converged(engine, s, 7, "B3LYP")[0]["P"]
    P = _CONVERGED["co"]
    rng = np.random.default_rng(3)
    D = rng.standard_normal(P.shape)
    D = 0.5 * (D + D.T) / np.abs(D).max()
    xid, cid, dfx, dfc, _ = _ids(name)
    assert _raw_setup(engine, s.pts, s.wts, xid, cid, dfx, dfc) == 0
    _, V, _, _, _ = _vxc_rc(engine, P)
    lin = float(np.sum(V * D))
    for h in (1e-3, 1e-4, 1e-5):
        ep = sum(_vxc_rc(engine, P + h * D)[3:])
        em = sum(_vxc_rc(engine, P - h * D)[3:])
        fd = (ep - em) / (2 * h)
        print(f"MEASURED gradient {name} h={h:g}: {abs(fd - lin) / abs(lin):.2e}")
    assert abs(fd - lin) < 2e-9 * abs(lin)
    engine.dft_clear()


# ---- converged KS state without a golden ---------------------------------------------------------------------------------------

def test_converged_b3lyp_n2_ccpvqz_energy_and_stationarity(engine):
    """B3LYP / N2 / cc-pVQZ on the medium grid, extreme convergence: the energy rebuilt from tr(PH), J and K of fock_jk and the reference's
    E_XC, and the commutator X^T (F P S - S P F) X of F = H + J - hfx/2 K + V_XC(reference) at the cycle's threshold.
    Measured: |dE| 6.8e-13 Eh (bar 1e-11), commutator 2.1e-12 (threshold 1e-9)."""
    from oracle import scf_oracle as so
    from tuna_amd.engine import SCF_CONVERGENCE
    s = System(engine, ["N", "N"], R_N2, "cc-pVQZ", True, "medium")
    f = engine.dft_setup(s.pts, s.wts, "B3LYP")
    xyz, chg = [a.origin for a in s.atoms], [7.0, 7.0]
    S, T, Vn, _, _ = engine.one_electron(xyz, chg, [0, 0, 0.0])
    X, _, _ = engine.orthogonaliser(S)
    P0, E0 = so.core_guess(T, Vn, X, 7)
    V_NN = mol.nuclear_repulsion(s.atoms)
    r = engine.scf_rhf(S, T, Vn, P0, E0, 7, V_NN, X=X, conv="extreme", damping="dynamic", hfx=f["hfx"])
    engine.dft_clear()
    P = r["P"]
    J, K = engine.fock_jk(P)
    xid, cid, dfx, dfc, hfx = _ids("B3LYP")
    Vx, n_el, ex, ec = s.ref(P, xid, cid, dfx, dfc)
    H = T + Vn
    E = np.sum(P * H) + 0.5 * np.sum(P * J) - hfx / 4.0 * np.sum(P * K) + ex + ec + V_NN
    F = H + J - hfx / 2.0 * K + Vx
    comm = np.abs(X.T @ (F @ P @ S - S @ P @ F) @ X).max()
    print(f"MEASURED converged N2/cc-pVQZ: dE {abs(E - r['energy']):.2e} comm {comm:.2e} n_el-14 {n_el - 14:.2e}")
    assert abs(E - r["energy"]) < 1e-11
    assert comm < SCF_CONVERGENCE["extreme"]["commutator"]


# ---- bitwise reproducibility and the error paths -------------------------------------------------------------------------------

def test_vxc_is_bitwise_reproducible(engine):
    s = System(engine, ["C", "O"], R_CO, "def2-TZVP", True, "medium")
    P = _random_densities(s.N, np.random.default_rng(5), 7)["psd"]
    engine.dft_setup(s.pts, s.wts, "B3LYP")
    a = engine.dft_vxc(P)
    b = engine.dft_vxc(P)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    engine.dft_clear()


def test_sph_matrix_is_the_references(engine):
    from conftest import HIGH_L_BASIS
    shells = mol.build_shells(mol.make_atoms(["N", "O"], 2.1), HIGH_L_BASIS)
    U = engine.set_basis(mol.expand_cartesian_aos(shells)).sph_matrix()
    np.testing.assert_array_equal(U, transformation_matrix([s.L for s in shells]))


def test_error_paths_leave_the_context_usable(engine):
    """tf_dft_vxc before tf_dft_setup, bad functional ids, the grid released by tf_set_basis and by tf_build_eri of the other AO
    representation, tf_scf_uhf and tf_scf_rhf_batch with a grid set: each is refused with TF_EINVAL, and a setup + V_XC afterwards
    gives the same bits as before."""
    from oracle import scf_oracle as so
    from tuna_amd._lib import TunaError
    s = System(engine, ["N", "N"], R_N2, "6-31G*", True, "loose")
    engine.dft_clear()
    P = _random_densities(s.N, np.random.default_rng(2), 7)["psd"]
    assert _vxc_rc(engine, P)[0] == TF_EINVAL                                  # before any setup
    for xid, cid in ((4, 0), (-1, 0), (0, 6), (0, -1)):
        assert _raw_setup(engine, s.pts, s.wts, xid, cid) == TF_EINVAL
        assert _vxc_rc(engine, P)[0] == TF_EINVAL
    engine.dft_setup(s.pts, s.wts, "B3LYP")
    good = engine.dft_vxc(P)
    engine.set_basis(s.aos)                                                    # tf_set_basis releases the grid
    assert _vxc_rc(engine, P)[0] == TF_EINVAL
    engine.build_eri(True)
    assert _vxc_rc(engine, P)[0] == TF_EINVAL
    engine.dft_setup(s.pts, s.wts, "B3LYP")
    engine.build_eri(False)                                                    # the Cartesian dimension differs: grid released
    assert engine.N != s.N
    assert _vxc_rc(engine, np.zeros((engine.N, engine.N)))[0] == TF_EINVAL
    engine.build_eri(True)
    engine.dft_setup(s.pts, s.wts, "B3LYP")
    xyz, chg = [a.origin for a in s.atoms], [7.0, 7.0]
    S, T, Vn, _, _ = engine.one_electron(xyz, chg, [0, 0, 0.0])
    X, _, _ = engine.orthogonaliser(S)
    P0, E0 = so.core_guess(T, Vn, X, 7)
    with pytest.raises(TunaError) as e:
        engine.scf_uhf(S, T, Vn, P0 / 2, P0 / 2, E0, 7, 7, 0.0, X=X)
    assert e.value.code == TF_EINVAL and "not implemented" in str(e.value)
    with pytest.raises(TunaError) as e:
        engine.scf_rhf_batch(S, T, Vn, [P0, P0], [E0, E0], 7, 0.0, X=X)
    assert e.value.code == TF_EINVAL and "tf_dft_clear" in str(e.value)
    again = engine.dft_vxc(P)
    assert np.array_equal(again[0], good[0]) and again[1:] == good[1:]
    engine.dft_clear()
