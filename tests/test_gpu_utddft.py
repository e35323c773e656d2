"""GPU: unrestricted TD-DFT / TDA and the Kohn-Sham stability analysis for the local-density functionals -- the spin-blocked kernel
build (tfxck::xck_spin_kernel and its slab sum through tf_xc_kernel_spin_probe), the spin-resolved point kernels
(tfdft::xc_fpoint2_kernel), the kernel matrix (tf_xc_kernel_uhf), the drivers (tf_tddft_uhf, tf_stability_rks, tf_stability_uks: the
shared assembly and solve stages of tf_cis_uhf and tf_stability_rhf / _uhf) -- against a float64 NumPy contraction, the NumPy model of
tests/xc_kernel_spin_reference.py, the restricted routines (a closed shell through the open-shell code), tf_cis_uhf bit for bit, and,
independent of all of them, the linear response of the unrestricted V_XC.  Every test that sets a grid clears it and hands the shared
context back with the default layout.

The bound of the probe is that of tests/test_gpu_xc_kernel_probe.py: an element is a sum of G terms u psi psi psi psi, either side
rounds three products per term and one addition per term in some order, so the two differ by at most 2 gamma_G S, S the sum of the
magnitudes of the terms.  Nothing in it is fitted to what the kernel returns.

Measured on one MI355X (the prints of these tests): the probe within 0.85 of its bound (at G = 1; 0.03 at G = 33, below 0.005 from
G = 256); the five point kernels within 3.1 eps of the sums of the magnitudes of their terms of the model at the device's own densities,
zeta from 0 to 1 - 2e-23 / rho; the spin densities within 1.4e-14 of the sums of the magnitudes of THEIR terms of the model's and within
7.5e-15 of the reference's; against the stored point kernels up to 0.99 of the first-order allowance; K within 1.0e-15 of the stored
matrices (5.5e-4 of the bound), the same bits on the three layouts; TDA energies within 1.4e-14 Eh, TD-DFT energies within 6.8e-12 Eh
(OH / STO-3G; tolerance 8.5e-11 there), cluster sums of |mu| within 6.7e-13 and of f within 2.8e-14; the lowest Hessian eigenvalues
within 5.2e-15 (unrestricted) and 2.6e-15 (restricted); a closed shell through the open-shell code within 2.3e-13 Eh of the restricted
spectrum; the linear-response identity within 2.2e-8, 2.6e-9, 2.4e-9 and 1.6e-8 of 2 K kappa in the aa, ba, ab and bb blocks, whose
largest elements are 0.16, 0.022, 0.0098 and 0.12, at h = 5e-4, against its own estimates of the stencil error 6.7e-8, 7.7e-9, 7.3e-9 and
4.9e-8; calculate_energy on NH / STO-3G UHFS within 1.2e-13 Eh of the golden energies; 64 x 64 and 64 x 128 tiles the same bits at
every probe shape; the unstable systems' Hessian eigenvalues (-0.078, -0.146) within the same bound, full TD-DFT refused."""
import numpy as np
import pytest

import xc_kernel_reference as xk
import xc_kernel_spin_reference as xs
from test_cis_reference import CIS_TOL, MOMENT_TOL, TDHF_TOL, cluster_sums, split
from test_gpu_mp3 import _reset
from test_ucis_reference import STAB_TOL, orbitals, usystem, windows
from test_ucis_reference import SYSTEMS as UCIS_SYSTEMS
from tuna_amd import molecule as mol
from tuna_amd._lib import TunaError
from tuna_amd.engine import Engine

pytestmark = pytest.mark.gpu

TF_EINVAL = -1
EPS = np.finfo(np.float64).eps
# (o_alpha, v_alpha, o_beta, v_beta): both spins ragged (63 + 63); d_alpha = 64 exactly and d_beta = 64 = one o; d_alpha = 65 (one element
# past a tile) with an empty beta block whose v is not 0; an empty alpha block; d_alpha = 129 (three alpha blocks, the last of one
# element) next to d_beta = 128; one element per spin
PROBE_SHAPES = [(7, 9, 9, 7), (8, 8, 1, 64), (1, 65, 0, 5), (0, 3, 5, 13), (3, 43, 2, 64), (1, 1, 1, 1)]
G_SLABS = 2500                        # nine slabs of 288 points, the last of 196 = six chunks and four points
PROBE_G = (1, 33, 256, G_SLABS)


@pytest.fixture
def eng(engine):
    """the shared context; whatever the test leaves, the grid is cleared and the layout is the default again"""
    yield engine
    engine.dft_clear()
    _reset(engine)


@pytest.fixture(scope="module")
def tddft_golden(golden):
    return xk.split(golden("tddft_systems"))


def probe_operands(oa, va, ob, vb, G):
    rng = np.random.default_rng(100000 * oa + 1000 * va + 100 * ob + vb + 7 * G)
    psi = [rng.standard_normal((n, G)) for n in (oa, va, ob, vb)]
    u = [rng.standard_normal(G) for _ in range(3)]
    return psi, u


@pytest.mark.parametrize("oa,va,ob,vb", PROBE_SHAPES)
def test_spin_probe_against_numpy(engine, oa, va, ob, vb):
    """tf_xc_kernel_spin_probe against xc_kernel_spin_reference.spin_kernel_matrix (float64 matmul) element by element within
    2 gamma_G S, with 64 x 64 and with 64 x 128 tiles (the same bits), K == K^T bitwise, a second call the same bits, and the alpha-beta
    rectangle NOT within the bound of a contraction with u_aa or u_bb in place of u_ab."""
    da, db = oa * va, ob * vb
    for G in PROBE_G:
        psi, u = probe_operands(oa, va, ob, vb, G)
        shapes = []
        for cols in (1, 2, 0):                                # 64 x 64 tiles, 64 x 128 tiles, the library's default (left set)
            engine.xc_kernel_spin_cols(cols)
            shapes.append(engine.xc_kernel_spin_probe(*psi, *u))
        K = shapes[-1]
        assert np.array_equal(shapes[0], shapes[1]) and np.array_equal(shapes[0], K)           # either shape: the same bits
        want, S = xs.spin_kernel_matrix(*psi, *u, with_magnitudes=True)
        plan = Engine.xc_kernel_spin_plan(da, db, G)
        gamma = G * EPS / (1 - G * EPS)
        assert K.shape == (da + db, da + db) and np.isfinite(K).all()
        ratio = (np.abs(K - want) / (2 * gamma * S)).max()
        print(f"\n[{oa} {va} {ob} {vb} G {G}] d_alpha {da} d_beta {db} blocks {plan['n_b_alpha']} + {plan['n_b_beta']} tiles {plan['n_tiles']} "
              f"slabs {plan['n_slabs']} x {plan['slab_len']} max |d| / (2 gamma_G S) = {ratio:.3f}")
        assert ratio <= 1.0
        assert np.array_equal(K, K.T)
        assert np.array_equal(engine.xc_kernel_spin_probe(*psi, *u), K)
        if da and db and G > 1:
            for wrong in (0, 2):
                other = xs.spin_kernel_matrix(*psi, u[0], u[wrong], u[2])
                assert np.any(np.abs(K[:da, da:] - other[:da, da:]) > 2 * gamma * S[:da, da:]), "the alpha-beta rectangle passes with the wrong weight"
    if G_SLABS in PROBE_G:
        p = Engine.xc_kernel_spin_plan(da, db, G_SLABS)
        assert p["n_slabs"] >= 3 and G_SLABS % p["slab_len"] != 0 and (G_SLABS % p["slab_len"]) % 32 != 0


def test_spin_probe_equal_spins_repeat_the_restricted_kernel(engine):
    """psi_alpha = psi_beta and one weight for the three: each of the four blocks is the restricted kernel's matrix -- not to the bit
    (the restricted kernel cuts its blocks of 64 through the whole index, this one per spin) but within the same bound."""
    o, v, G = 3, 30, 700
    psi, u = probe_operands(o, v, o, v, G)
    K = engine.xc_kernel_spin_probe(psi[0], psi[1], psi[0], psi[1], u[0], u[0], u[0])
    KS, _ = engine.xc_kernel_probe(psi[0], psi[1], u[0], u[0])
    d = o * v
    _, S = xs.spin_kernel_matrix(psi[0], psi[1], psi[0], psi[1], u[0], u[0], u[0], with_magnitudes=True)
    gamma = G * EPS / (1 - G * EPS)
    for blk in (K[:d, :d], K[:d, d:], K[d:, :d], K[d:, d:]):
        assert np.all(np.abs(blk - KS) <= 2 * gamma * S[:d, :d])
    assert np.array_equal(K[:d, :d], K[d:, d:])              # the two diagonal blocks run the same operations on the same values


def test_spin_probe_refusals(engine):
    psi, u = probe_operands(2, 3, 1, 4, 9)
    first = engine.xc_kernel_spin_probe(*psi, *u)
    L, ctx = engine._L, engine._ctx
    from tuna_amd._lib import ptr
    K = np.zeros((10, 10))
    p, w = [ptr(x) for x in psi], [ptr(x) for x in u]
    bad = [(0, 3, 0, 4, 9, *p, *w, ptr(K)), (2, 0, 1, 0, 9, *p, *w, ptr(K)), (-1, 3, 1, 4, 9, *p, *w, ptr(K)), (2, 3, 1, 4, 0, *p, *w, ptr(K)),
           (2, 3, 1, 4, 9, None, p[1], p[2], p[3], *w, ptr(K)), (2, 3, 1, 4, 9, *p, w[0], None, w[2], ptr(K)), (2, 3, 1, 4, 9, *p, *w, None)]
    for args in bad:
        assert L.tf_xc_kernel_spin_probe(ctx, *args) == TF_EINVAL, args
        assert "tf_xc_kernel_spin_probe" in L.tf_last_error(ctx).decode()
    assert np.array_equal(engine.xc_kernel_spin_probe(*psi, *u), first)                   # the context stays usable
    assert L.tf_xc_kernel_spin_probe(ctx, 2, 3, 0, 4, 9, p[0], p[1], None, None, *w, ptr(K)) == 0      # an empty spin needs no pointers
    assert np.array_equal(K.ravel()[:36].reshape(6, 6), first[:6, :6])
    with pytest.raises(ValueError):
        engine.xc_kernel_spin_probe(psi[0], psi[1][:, :5], psi[2], psi[3], *u)
    with pytest.raises(TunaError):
        Engine.xc_kernel_spin_plan(0, 0, 5)


def setup(engine, tag, functional="golden", layout=None):
    r = xk.rebuilt(tag)
    engine.set_basis(r["aos"]).build_eri(True, layout=layout)
    engine.dft_setup(r["pts"], r["wts"], xk.SYSTEMS[tag][4] if functional == "golden" else functional)
    return r


def open_shell_of(g, n_alpha, n_beta):
    """An open-shell determinant from closed-shell orbitals: C_alpha = C_beta = C, the lowest n_alpha / n_beta occupied"""
    C = g["C"]
    return C, C, C[:, :n_alpha] @ C[:, :n_alpha].T, C[:, :n_beta] @ C[:, :n_beta].T


@pytest.mark.parametrize("tag", ["lih_hfs_sto3g", "lih_svwn3_sto3g", "hf_svwn_631g"])
def test_point_kernels_against_the_model(eng, tddft_golden, tag):
    """f_points of tf_xc_kernel_uhf on the whole grid of a stored system, closed shell (rho_alpha = rho_beta: zeta = 0 exactly) and with
    an electron moved from beta to alpha (every zeta in between, |zeta| -> 1 in the tail of the alpha HOMO), against the model at the
    device's own densities within POINT_TOL = 64 eps of the sums of the magnitudes of the terms; the densities against the model's
    within RHO_TOL of theirs.  At zeta = 0, f_aa + f_ab and f_aa - f_ab are the restricted singlet and triplet kernels of the device."""
    g = tddft_golden[tag]
    r = setup(eng, tag)
    functional = xk.SYSTEMS[tag][4]
    nocc = int(g["n_occ"])
    for na, nb in ((nocc, nocc), (nocc + 1, nocc - 1)):
        Ca, Cb, Pa, Pb = open_shell_of(g, na, nb)
        K, fp = eng.xc_kernel_uhf(Ca, Cb, Pa, Pb, na, nb, return_points=True)
        G = len(r["wts"])
        assert fp.shape == (7, G) and np.isfinite(fp).all() and fp[:2].min() >= xs.FLOOR
        for s, P in enumerate((Pa, Pb)):
            rho, mag = xk.density(r["phi"], P)
            d = np.abs(fp[s] - np.maximum(rho, xs.FLOOR)) / mag
            assert d.max() <= xk.RHO_TOL, (s, d.max())
        pk = xs.point_kernels(fp[0], fp[1], functional, floored=True)
        worst = {}
        for row, k in enumerate(("f_X_aa", "f_X_bb", "f_C_aa", "f_C_ab", "f_C_bb"), start=2):
            d = np.abs(fp[row] - pk[k])
            worst[k] = np.max(d / np.maximum(pk["mag_" + k], 1e-300)) / EPS
            assert np.all(d <= xs.POINT_TOL * pk["mag_" + k]), (k, worst[k])
        z = (fp[0] - fp[1]) / (fp[0] + fp[1])
        print(f"\n[{tag} ({na}, {nb})] G {G} zeta in [{z.min():.3f}, {z.max():.3f}] max |d| / mag in eps: " + ", ".join(f"{k} {x:.1f}" for k, x in worst.items()))
        if functional == "HFS":
            assert not fp[4:].any()
        if na == nb:
            KS, KT, fr = eng.xc_kernel_rhf(g["C"], g["P"], nocc, 0, return_points=True)
            pr = xk.point_kernels(fr[0], functional)
            tolS = xs.POINT_TOL * (pk["mag_f_X_aa"] + pk["mag_f_C_aa"] + pk["mag_f_C_ab"] + pr["mag_X"] + pr["mag_CS"])
            tolT = xs.POINT_TOL * (pk["mag_f_X_aa"] + pk["mag_f_C_aa"] + pk["mag_f_C_ab"] + pr["mag_X"] + pr["mag_CT"])
            # the two routines sum the density in different orders: the first-order effect of the difference is allowed, |df / drho| |d rho|;
            # points where a density sits at its floor are left out (the floors differ: 1e-23 per spin against 1e-23 in all)
            h = 1e-6
            up, dn = xk.point_kernels(fr[0] * (1 + h), functional), xk.point_kernels(fr[0] * (1 - h), functional)
            d_rho = np.abs(fp[0] + fp[1] - fr[0])
            live = (fr[0] > 2 * xs.FLOOR) & (fp[0] > xs.FLOOR) & (fp[1] > xs.FLOOR)
            assert live.mean() > 0.5                              # (the comparison is not vacuous)
            for c, row, tol in (("f_CS", 2, tolS), ("f_CT", 3, tolT)):
                slope = np.abs(up["f_X"] + up[c] - dn["f_X"] - dn[c]) / (2 * h * fr[0])
                got = fp[2] + fp[4] + (fp[5] if c == "f_CS" else -fp[5])
                assert np.all(np.abs(got - fr[1] - fr[row])[live] <= (tol + 1.01 * slope * d_rho)[live]), c


@pytest.mark.parametrize("tag", ["li_svwn3_631g", "oh_lda_sto3g", "h_lda_631g"])
def test_spins_exchanged(eng, golden, tag):
    """The stored open-shell solutions with alpha and beta exchanged in the call (C_beta, P_beta, n_beta passed as alpha): now
    the majority spin is beta, zeta runs down to -1 (H: rho_alpha at the floor on the whole grid, d_alpha = 0), and the other branches of the
    clip and of the floors in f''(zeta) are the ones taken.  The point kernels against the model at the device's densities within
    POINT_TOL of the magnitudes; the densities are the unexchanged call's; K is that call's matrix with its spin blocks exchanged, each
    within the model's bound of the exact one."""
    g = xk.split(golden("utddft_systems"))[tag]
    functional = xs.SYSTEMS[tag][5]
    r = xs.rebuilt(tag)
    eng.set_basis(r["aos"]).build_eri(True)
    eng.dft_setup(r["pts"], r["wts"], functional)
    na, nb = int(g["n_alpha"]), int(g["n_beta"])
    K, fp = eng.xc_kernel_uhf(g["C_alpha"], g["C_beta"], g["P_alpha"], g["P_beta"], na, nb, return_points=True)
    Kx, fx = eng.xc_kernel_uhf(g["C_beta"], g["C_alpha"], g["P_beta"], g["P_alpha"], nb, na, return_points=True)
    z, z0 = (fx[0] - fx[1]) / (fx[0] + fx[1]), (fp[0] - fp[1]) / (fp[0] + fp[1])
    assert np.isfinite(fx).all() and z0.max() > 0 and z.min() <= -z0.max() + 1e-9          # zeta is the unexchanged call's with its sign turned
    pk = xs.point_kernels(fx[0], fx[1], functional, floored=True)
    for row, k in enumerate(("f_X_aa", "f_X_bb", "f_C_aa", "f_C_ab", "f_C_bb"), start=2):
        assert np.all(np.abs(fx[row] - pk[k]) <= xs.POINT_TOL * pk["mag_" + k]), k
    for s_, t_ in ((0, 1), (1, 0)):                          # the densities are the unexchanged call's, within their own bound
        rho, mag = xk.density(r["phi"], g["P_beta"] if s_ == 0 else g["P_alpha"])
        assert np.all(np.abs(fx[s_] - fp[t_]) <= 2 * xk.RHO_TOL * np.maximum(mag, xs.FLOOR))
    N = len(g["eps_alpha"])
    da = na * (N - na)
    want = np.block([[K[da:, da:], K[da:, :da]], [K[:da, da:], K[:da, :da]]])
    m = xs.golden_model(tag, g, 0)
    b = xs.k_bound(m)
    bound = np.block([[b[da:, da:], b[da:, :da]], [b[:da, da:], b[:da, :da]]])
    assert Kx.shape == want.shape and np.all(np.abs(Kx - want) <= 2 * bound) and np.array_equal(Kx, Kx.T)


@pytest.mark.parametrize("tag", ["lih_svwn3_sto3g", "hf_svwn_631g"])
def test_closed_shell_through_the_open_shell_code(eng, tddft_golden, tag):
    """C_alpha = C_beta, P_alpha = P_beta = P / 2 of a stored closed-shell Kohn-Sham solution: the spin-blocked matrices are orthogonally
    similar to diag(singlet, triplet) of the restricted routine, so the spectrum of tf_tddft_uhf is the union of tf_tddft_rhf's singlets
    and triplets and tf_stability_uks's lowest eigenvalue the smaller of tf_stability_rks's two.  Allowed: the bounds of
    test_gpu_cis.py for the two solves plus the spectral effect of the kernels' rounding, twice the Frobenius norm of the element-wise
    bound of either kernel matrix (k_bounds of test_gpu_tddft.py; each route is within its bound of the exact matrix).  |mu| and f: the
    singlets carry the restricted routine's, the triplets none."""
    g = tddft_golden[tag]
    setup(eng, tag)
    nocc = int(g["n_occ"])
    C, eps, P = g["C"], g["eps"], g["P"]
    for nf in xk.frozen_variants(g):
        m = xk.model_kernel(tag, g, nf)
        g2 = 2 * xk.gamma(m["G"])
        dK = 2 * (np.linalg.norm(g2 * m["SS"] + xk.RHO_TOL * m["DS"]) + np.linalg.norm(g2 * m["ST"] + xk.RHO_TOL * m["DT"]))
        for method, base in (("TDA", CIS_TOL), ("TDDFT", TDHF_TOL)):
            r = eng.tddft_rhf(C, eps, P, nocc, nf, method=method, dip=g["dip"])
            u = eng.tddft_uhf(C, C, eps, eps, P / 2, P / 2, nocc, nocc, nf, nf, method=method, dip=g["dip"])
            both = np.concatenate([r["E_singlet"], r["E_triplet"]])
            order = np.argsort(both, kind="stable")
            d = np.abs(u["E"] - both[order]).max()
            mu = np.concatenate([np.linalg.norm(r["tdm"], axis=1), np.zeros(len(r["E_triplet"]))])[order]
            f = np.concatenate([r["osc"], np.zeros(len(r["E_triplet"]))])[order]
            d_mu = np.abs(cluster_sums(both[order], np.linalg.norm(u["tdm"], axis=1)) - cluster_sums(both[order], mu)).max()
            d_f = np.abs(cluster_sums(both[order], u["osc"]) - cluster_sums(both[order], f)).max()
            print(f"\n[{tag} {method} fc{nf}] dim {u['dim']} max |E_uhf - sorted(E_S u E_T)| {d:.1e} (tol {2 * base + dK:.1e}, of which the kernels {dK:.1e}) "
                  f"cluster |mu| d {d_mu:.1e} f d {d_f:.1e}")
            assert u["dim"] == 2 * r["dim"] and u["dim_alpha"] == r["dim"]
            assert d <= 2 * base + dK and d_mu <= MOMENT_TOL and d_f <= MOMENT_TOL
        s = eng.stability_rks(C, eps, P, nocc, nf)
        su = eng.stability_uks(C, C, eps, eps, P / 2, P / 2, nocc, nocc, nf, nf)
        want = min(s["lowest_singlet"], s["lowest_triplet"])
        print(f"[{tag} fc{nf}] lowest Hessian eigenvalues: restricted singlet {s['lowest_singlet']:.8f} ({s['source_singlet']}) triplet "
              f"{s['lowest_triplet']:.8f} ({s['source_triplet']}); unrestricted {su['lowest']:.8f} ({su['source']})")
        assert abs(su["lowest"] - want) <= 2 * STAB_TOL + 2 * dK and su["dim"] == 2 * s["dim"]


def test_kernel_shifts_the_stability_eigenvalues(eng, tddft_golden):
    """tf_stability_rks on HF/6-31G SVWN against NumPy: eigvalsh of tddft_rhf's returned A + B (singlet, triplet) and A - B, which carry
    2 K_S, 2 K_T and nothing; and the same numbers differ from the kernel-free ones (functional None, hfx = 0) by more than the bound."""
    tag = "hf_svwn_631g"
    g = tddft_golden[tag]
    r = setup(eng, tag)
    nocc = int(g["n_occ"])
    C, eps, P = g["C"], g["eps"], g["P"]
    t = eng.tddft_rhf(C, eps, P, nocc, 0, method="TDDFT", return_matrices=True)
    s = eng.stability_rks(C, eps, P, nocc, 0, return_spectra=True)
    for name, key in (("plus_singlet", "M_plus_singlet"), ("plus_triplet", "M_plus_triplet"), ("minus", "M_minus")):
        d = np.abs(s["spectra"][name] - np.linalg.eigvalsh(t[key])).max()
        print(f"\n[{name}] max |eig - eigvalsh(matrix of tddft_rhf)| {d:.1e}")
        assert d <= STAB_TOL
    assert s["lowest_singlet"] == min(s["spectra"]["plus_singlet"][0], s["spectra"]["minus"][0])
    eng.dft_setup(r["pts"], r["wts"], None)
    bare = eng.stability_rks(C, eps, P, nocc, 0, hfx=0.0)
    assert abs(bare["lowest_singlet"] - s["lowest_singlet"]) > 1e-3 or abs(bare["lowest_triplet"] - s["lowest_triplet"]) > 1e-3
    hf = eng.stability_rhf(C, eps, nocc, 0)                   # the null functional with hfx = 1 is the Hartree-Fock routine
    same = eng.stability_rks(C, eps, P, nocc, 0, hfx=1.0)
    assert same["lowest_singlet"] == hf["lowest_singlet"] and same["lowest_triplet"] == hf["lowest_triplet"]


@pytest.fixture(scope="module")
def ucis_golden(golden):
    return split(golden("ucis_systems"))


@pytest.mark.parametrize("tag", ["li_doublet_631g", "o2_triplet_sto3g", "h_ccpvdz"])
def test_null_functional_is_cis_uhf_bit_for_bit(eng, ucis_golden, tag):
    """tf_dft_setup with exchange and correlation ids 0 and hfx = 1: no kernel is built, the exchange blocks are multiplied by 1.0, and
    every output of tddft_uhf -- energies, vectors, moments, the assembled matrices -- is cis_uhf's, CIS and TDHF, to the last bit; a
    second tddft_uhf call equals the first; stability_uks equals stability_uhf.  H (1, 0) has an empty beta block.  Where TDHF refuses
    the reference as unstable (O2/STO-3G), TD-DFT refuses it with the same message under its own name."""
    from tuna_amd import dft
    g = ucis_golden[tag]
    sym, R, basis = UCIS_SYSTEMS[tag]
    atoms = mol.make_atoms(sym, R)
    eng.set_basis(usystem(tag)[1]).build_eri(True)
    pts, wts, _ = dft.integration_grid(atoms, "loose")
    f = eng.dft_setup(np.asarray(pts, float).reshape(3, -1), np.asarray(wts, float).reshape(-1), None)
    assert f["hfx"] == 1.0 and f["name"] == "NONE"
    Ca, Cb, ea, eb = orbitals(g)
    na, nb, nfa, nfb = windows(g)
    Pa, Pb = Ca[:, :na] @ Ca[:, :na].T, Cb[:, :nb] @ Cb[:, :nb].T
    for cis_name, td_name in (("CIS", "TDA"), ("TDHF", "TDDFT")):
        try:
            a = eng.cis_uhf(Ca, Cb, ea, eb, na, nb, nfa, nfb, method=cis_name, n_keep=5, dip=g["dip"], return_matrices=True)
        except TunaError as e:
            with pytest.raises(TunaError) as e2:
                eng.tddft_uhf(Ca, Cb, ea, eb, Pa, Pb, na, nb, nfa, nfb, method=td_name, n_keep=5, dip=g["dip"])
            assert e2.value.code == e.code and str(e2.value).replace("tf_tddft_uhf", "tf_cis_uhf") == str(e)
            continue
        b = eng.tddft_uhf(Ca, Cb, ea, eb, Pa, Pb, na, nb, nfa, nfb, method=td_name, n_keep=5, dip=g["dip"], return_matrices=True)
        c = eng.tddft_uhf(Ca, Cb, ea, eb, Pa, Pb, na, nb, nfa, nfb, method=td_name, n_keep=5, dip=g["dip"], return_matrices=True)
        assert set(a) == set(b)
        for key in a:
            if key == "seconds":
                continue
            if a[key] is None:
                assert b[key] is None, key
            else:
                assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (cis_name, key)
                assert np.asarray(c[key]).tobytes() == np.asarray(b[key]).tobytes(), (td_name, key)
    K = eng.xc_kernel_uhf(Ca, Cb, Pa, Pb, na, nb, nfa, nfb)                                    # the kernel of nothing is nothing
    assert not K.any()
    s, su = eng.stability_uhf(Ca, Cb, ea, eb, na, nb, nfa, nfb), eng.stability_uks(Ca, Cb, ea, eb, Pa, Pb, na, nb, nfa, nfb)
    assert s["lowest"] == su["lowest"] and s["source"] == su["source"]


def test_second_call_and_layouts_give_the_same_bits(eng, tddft_golden):
    """With a functional: K of an open-shell determinant and the TD-DFT energies, a second call and the three tensor layouts (the kernel
    build does not read the tensor; the MO blocks do)."""
    tag = "hf_svwn_631g"
    g = tddft_golden[tag]
    nocc = int(g["n_occ"])
    Ca, Cb, Pa, Pb = open_shell_of(g, nocc + 1, nocc - 1)
    eps = g["eps"]
    first = None
    for layout in ("packed", "rows", "tiles"):
        setup(eng, tag, layout=layout)
        K = eng.xc_kernel_uhf(Ca, Cb, Pa, Pb, nocc + 1, nocc - 1, 1, 1)
        assert np.array_equal(K, K.T) and np.array_equal(K, eng.xc_kernel_uhf(Ca, Cb, Pa, Pb, nocc + 1, nocc - 1, 1, 1))
        r = eng.tddft_uhf(Ca, Cb, eps, eps, Pa, Pb, nocc + 1, nocc - 1, 1, 1, method="TDA", return_matrices=True)
        assert np.array_equal(r["M_plus"], r["M_plus"].T)
        again = eng.tddft_uhf(Ca, Cb, eps, eps, Pa, Pb, nocc + 1, nocc - 1, 1, 1, method="TDA", return_matrices=True)
        assert np.array_equal(r["E"], again["E"]) and np.array_equal(r["M_plus"], again["M_plus"])
        if first is None:
            first = K
        assert np.array_equal(K, first), layout


def test_assembly_with_the_kernel(eng, golden):
    """The assembled matrices against a NumPy assembly from ao_to_mo's blocks and xc_kernel_uhf's K, on the stored unrestricted Kohn-Sham
    solution of NH / STO-3G SVWN3 with one frozen orbital per spin:
        A = d_st (Delta - hfx H) + G + K,   A + B = d_st (Delta - hfx H - hfx X) + 2 G + 2 K,   A - B = d_st (Delta - hfx H + hfx X).
    hfx = 0 (the functional's own): the returned matrices of TDA and TD-DFT within 1e-11 of the largest entry (test_gpu_cis.py's bar for
    the same matrices), A - B the diagonal exactly.  hfx = 0.25: A of TDA likewise, and -- whether or not that Hessian is positive
    definite -- the spectra of A + B and A - B from stability_uks against eigvalsh of the NumPy matrices within STAB_TOL."""
    tag = "nh_svwn3_sto3g"
    g = xk.split(golden("utddft_systems"))[tag]
    r = xs.rebuilt(tag)
    eng.set_basis(r["aos"]).build_eri(True)
    eng.dft_setup(r["pts"], r["wts"], xs.SYSTEMS[tag][5])
    na, nb, nf = int(g["n_alpha"]), int(g["n_beta"]), 1
    Ca, Cb, ea, eb, Pa, Pb = g["C_alpha"], g["C_beta"], g["eps_alpha"], g["eps_beta"], g["P_alpha"], g["P_beta"]
    K = eng.xc_kernel_uhf(Ca, Cb, Pa, Pb, na, nb, nf, nf)
    Co, Cv, e = [Ca[:, nf:na], Cb[:, nf:nb]], [Ca[:, na:], Cb[:, nb:]], (ea, eb)
    d = [Co[s].shape[1] * Cv[s].shape[1] for s in range(2)]
    dim, off = sum(d), [0, d[0]]
    Gm, H, X, D = (np.zeros((dim, dim)) for _ in range(4))
    for s in range(2):
        for t in range(2):
            Gm[off[s]:off[s] + d[s], off[t]:off[t] + d[t]] = eng.ao_to_mo(Co[s], Cv[s], Co[t], Cv[t]).reshape(d[s], d[t])
        sl = slice(off[s], off[s] + d[s])
        X[sl, sl] = eng.ao_to_mo(Co[s], Cv[s], Co[s], Cv[s]).transpose(0, 3, 2, 1).reshape(d[s], d[s])
        H[sl, sl] = eng.ao_to_mo(Co[s], Co[s], Cv[s], Cv[s]).transpose(0, 2, 1, 3).reshape(d[s], d[s])
        n_s = (na, nb)[s]
        D[sl, sl] = np.diag((e[s][n_s:][None, :] - e[s][nf:n_s][:, None]).ravel())
    assert np.abs(K).max() > 1e-3 and np.abs(K[:d[0], d[0]:]).max() > 1e-4

    def sym(M):
        return 0.5 * (M + M.T)

    def close(got, M, what):
        dd = np.abs(got - M).max() / np.abs(M).max()
        print(f"\n[{what}] max |d| / max |entry| {dd:.1e}")
        assert dd <= 1e-11 and np.array_equal(got, got.T)
    for hfx in (0.0, 0.25):
        got = eng.tddft_uhf(Ca, Cb, ea, eb, Pa, Pb, na, nb, nf, nf, method="TDA", hfx=hfx, return_matrices=True)
        close(got["M_plus"], sym(D - hfx * H + Gm + K), f"hfx {hfx} TDA A")
        plus, minus = sym(D - hfx * (H + X) + 2 * Gm + 2 * K), sym(D - hfx * (H - X))
        st = eng.stability_uks(Ca, Cb, ea, eb, Pa, Pb, na, nb, nf, nf, hfx=hfx, return_spectra=True)
        for name, M in (("plus", plus), ("minus", minus)):
            dd = np.abs(st["spectra"][name] - np.linalg.eigvalsh(M)).max()
            print(f"[hfx {hfx} eig(A {'+' if name == 'plus' else '-'} B)] max |d| {dd:.1e}")
            assert dd <= STAB_TOL
    got = eng.tddft_uhf(Ca, Cb, ea, eb, Pa, Pb, na, nb, nf, nf, method="TDDFT", hfx=0.0, return_matrices=True)
    close(got["M_plus"], sym(D + 2 * Gm + 2 * K), "hfx 0.0 TDDFT A + B")
    assert np.array_equal(got["M_minus"], D)


def test_linear_response_identity(eng, tddft_golden):
    """Independent of the reference and of the model: K kappa against the central difference of the unrestricted V_XC, HF/6-31G SVWN
    orbitals occupied (6, 4).

    P_s = C_os C_os^T.  Rotating the occupied alpha orbitals by kappa [o_a, v_a], C_o -> C_o + C_v kappa^T, changes P_alpha by
    dP = C_v kappa^T C_o^T + C_o kappa C_v^T to first order and rho_alpha by d rho = 2 sum_jb kappa_jb psi_j psi_b; rho_beta stays.
    V_XC^s = int w (dF / d rho_s) phi phi with F the energy density per volume, so
        [C_oa^T (dV_alpha / dh) C_va]_ia = sum_g w F_aa psi_i psi_a 2 sum_jb kappa_jb psi_j psi_b = 2 (K_aa kappa)_ia,
        [C_ob^T (dV_beta / dh) C_vb]_ia = 2 (K_ba kappa)_ia,
    with u_aa = w F_aa (exchange: E_X = (E_X[2 rho_a] + E_X[2 rho_b]) / 2, so F_aa = 2 f_X(2 rho_a)) and u_ab = w F_ab; likewise for a
    rotation of the beta orbitals.  A kernel with the restricted factor of 2, or with u_aa in the rectangle, misses by |K kappa| itself.
    The tolerance is the stencil's own error estimate from two step sizes, as in test_gpu_tddft.py."""
    tag = "hf_svwn_631g"
    g = tddft_golden[tag]
    setup(eng, tag)
    nocc = int(g["n_occ"])
    na, nb = nocc + 1, nocc - 1
    Ca, Cb, Pa, Pb = open_shell_of(g, na, nb)
    C = g["C"]
    Co, Cv = (C[:, :na], C[:, :nb]), (C[:, na:], C[:, nb:])
    d = (na * Cv[0].shape[1], nb * Cv[1].shape[1])
    K = eng.xc_kernel_uhf(Ca, Cb, Pa, Pb, na, nb)
    v_max = max(np.abs(V).max() for V in eng.dft_vxc_unrestricted(Pa, Pb)[:2])
    for s in range(2):
        kappa = np.random.default_rng(21 + s).standard_normal((Co[s].shape[1], Cv[s].shape[1]))
        kappa /= np.abs(kappa).max()
        dP = Cv[s] @ kappa.T @ Co[s].T + Co[s] @ kappa @ Cv[s].T

        def quotient(h):
            P = [Pa, Pb]
            up, dn = list(P), list(P)
            up[s], dn[s] = P[s] + h * dP, P[s] - h * dP
            Vu, Vd = eng.dft_vxc_unrestricted(*up), eng.dft_vxc_unrestricted(*dn)
            return [Co[t].T @ ((Vu[t] - Vd[t]) / (2 * h)) @ Cv[t] for t in range(2)]
        h = 1e-3
        coarse, fine = quotient(h), quotient(h / 2)
        col = slice(0, d[0]) if s == 0 else slice(d[0], d[0] + d[1])
        for t in range(2):
            row = slice(0, d[0]) if t == 0 else slice(d[0], d[0] + d[1])
            want = 2 * (K[row, col] @ kappa.ravel()).reshape(Co[t].shape[1], Cv[t].shape[1])
            stencil = np.abs(coarse[t] - fine[t]).max()
            tol = stencil + 8 * EPS * v_max / (h / 2)
            dd = np.abs(fine[t] - want).max()
            print(f"\n[rotate {'ab'[s]}, block {'ab'[t]}{'ab'[s]}] max |2 K kappa| {np.abs(want).max():.3e} max |D(h/2) - 2 K kappa| {dd:.1e} stencil estimate {stencil:.1e} tol {tol:.1e}")
            assert dd <= tol and tol < 1e-4 * np.abs(want).max()
            assert np.abs(fine[t] - 2 * want).max() > 100 * tol and np.abs(fine[t] - 0.5 * want).max() > 100 * tol      # a factor of 2 would show


def test_refusals(eng, tddft_golden):
    tag = "hf_svwn_631g"
    g = tddft_golden[tag]
    r = setup(eng, tag)
    nocc = int(g["n_occ"])
    N = len(g["eps"])
    na, nb = nocc + 1, nocc - 1
    Ca, Cb, Pa, Pb = open_shell_of(g, na, nb)
    eps = g["eps"]
    first = eng.tddft_uhf(Ca, Cb, eps, eps, Pa, Pb, na, nb, method="TDA")

    def still_usable():
        again = eng.tddft_uhf(Ca, Cb, eps, eps, Pa, Pb, na, nb, method="TDA")
        assert np.array_equal(again["E"], first["E"])
    names = ("tf_tddft_uhf", "tf_xc_kernel_uhf", "tf_stability_uks", "tf_stability_rks")
    for call in (lambda: eng.tddft_uhf(Ca, Cb, eps, eps, None, Pb, na, nb), lambda: eng.tddft_uhf(Ca, Cb, eps, eps, Pa, None, na, nb),
                 lambda: eng.xc_kernel_uhf(Ca, Cb, Pa, None, na, nb), lambda: eng.stability_uks(Ca, Cb, eps, eps, None, Pb, na, nb),
                 lambda: eng.stability_rks(g["C"], eps, None, nocc),
                 lambda: eng.tddft_uhf(Ca, Cb, eps, eps, Pa, Pb, na, nb, na + 1, 0),              # n_frozen > n
                 lambda: eng.tddft_uhf(Ca, Cb, eps, eps, Pa, Pb, N + 1, nb),                      # n > N
                 lambda: eng.tddft_uhf(Ca, Cb, eps, eps, Pa, Pb, N, N),                           # d_alpha + d_beta = 0: no virtual orbital
                 lambda: eng.tddft_uhf(Ca, Cb, eps, eps, Pa, Pb, na, nb, na, nb),                 # d_alpha + d_beta = 0: every orbital frozen
                 lambda: eng.xc_kernel_uhf(Ca, Cb, Pa, Pb, 0, 0), lambda: eng.stability_uks(Ca, Cb, eps, eps, Pa, Pb, N, N),
                 lambda: eng.stability_rks(g["C"], eps, g["P"], nocc, nocc),
                 lambda: eng.tddft_uhf(Ca, Cb, eps, eps, Pa, Pb, na, nb, n_keep=-1),
                 lambda: eng.tddft_uhf(Ca, Cb, eps, eps, Pa, Pb, na, nb, hfx=float("nan")),
                 lambda: eng.stability_uks(Ca, Cb, eps, eps, Pa, Pb, na, nb, hfx=float("inf")),
                 lambda: eng.stability_rks(g["C"], eps, g["P"], nocc, hfx=float("nan"))):
        with pytest.raises(TunaError) as e:
            call()
        assert e.value.code == TF_EINVAL and any(n in str(e.value) for n in names), str(e.value)
        still_usable()
    # a gradient-corrected functional: the message names it
    for functional, parts in (("B3LYP", ("B3", "3P")), ("BLYP", ("B88", "LYP")), ("SLYP", ("Slater", "LYP"))):
        eng.dft_setup(r["pts"], r["wts"], functional)
        for call in (lambda: eng.tddft_uhf(Ca, Cb, eps, eps, Pa, Pb, na, nb), lambda: eng.xc_kernel_uhf(Ca, Cb, Pa, Pb, na, nb),
                     lambda: eng.stability_uks(Ca, Cb, eps, eps, Pa, Pb, na, nb), lambda: eng.stability_rks(g["C"], eps, g["P"], nocc)):
            with pytest.raises(TunaError, match="exchange-correlation kernel") as e:
                call()
            assert e.value.code == TF_EINVAL and all(n in str(e.value) for n in parts), str(e.value)
    eng.dft_setup(r["pts"], r["wts"], "SVWN")
    still_usable()
    # without a grid
    eng.dft_clear()
    for call in (lambda: eng.tddft_uhf(Ca, Cb, eps, eps, Pa, Pb, na, nb), lambda: eng.xc_kernel_uhf(Ca, Cb, Pa, Pb, na, nb),
                 lambda: eng.stability_uks(Ca, Cb, eps, eps, Pa, Pb, na, nb), lambda: eng.stability_rks(g["C"], eps, g["P"], nocc)):
        with pytest.raises(TunaError, match="tf_dft_setup") as e:
            call()
        assert e.value.code == TF_EINVAL
    ok = eng.cis_uhf(Ca, Cb, eps, eps, na, nb, method="CIS")                                  # the context stays usable
    assert ok["dim"] == first["dim"]


# ---- against the reference program's own numbers (tests/golden/utddft_systems.npz, utddft_text.json) ---------------------------------

@pytest.fixture(scope="module")
def utddft_golden(golden):
    return xk.split(golden("utddft_systems"))


def usetup(engine, tag, layout=None):
    r = xs.rebuilt(tag)
    engine.set_basis(r["aos"]).build_eri(True, layout=layout)
    engine.dft_setup(r["pts"], r["wts"], xs.SYSTEMS[tag][5])
    return r


def spin_orbitals(g):
    return g["C_alpha"], g["C_beta"], g["eps_alpha"], g["eps_beta"]


@pytest.mark.parametrize("tag", list(xs.SYSTEMS))
def test_point_kernels_at_the_picked_points(eng, utddft_golden, tag):
    """f_points of the golden systems: the spin densities within RHO_TOL of the sums of the magnitudes of their terms of the model's
    and, at the 400 picked points, of the reference's; each kernel against the model AT THE DEVICE'S densities within POINT_TOL of the
    sums of the magnitudes of its terms on the whole grid; and against the STORED values with the first-order effect of the densities'
    differences added, sum_s |df / d rho_s| |rho_s - rho_s,ref| -- both as test_gpu_tddft.py does for the restricted kernels."""
    g = utddft_golden[tag]
    functional = xs.SYSTEMS[tag][5]
    r = usetup(eng, tag)
    na, nb = int(g["n_alpha"]), int(g["n_beta"])
    K, fp = eng.xc_kernel_uhf(g["C_alpha"], g["C_beta"], g["P_alpha"], g["P_beta"], na, nb, return_points=True)
    pick = g["pick"]
    G = len(r["wts"])
    assert fp.shape == (7, G) and np.isfinite(fp).all() and fp[:2].min() >= xs.FLOOR
    for s, (P, key) in enumerate(((g["P_alpha"], "rho_a_pick"), (g["P_beta"], "rho_b_pick"))):
        rho, mag = xk.density(r["phi"], P)
        mag = np.maximum(mag, xs.FLOOR)                       # (an empty spin: rho = 0 exactly, floored on both sides)
        d_model = np.abs(fp[s] - np.maximum(rho, xs.FLOOR)) / mag
        d_ref = np.abs(fp[s][pick] - g[key]) / mag[pick]
        print(f"\n[{tag} rho_{'ab'[s]}] max |rho - model| / rho_mag {d_model.max():.1e}, |rho - reference| / rho_mag at the picks {d_ref.max():.1e} (tol {xk.RHO_TOL:.0e})")
        assert d_model.max() <= xk.RHO_TOL and d_ref.max() <= xk.RHO_TOL
    pk = xs.point_kernels(fp[0], fp[1], functional, floored=True)
    h = 1e-6
    ra, rb = fp[0][pick], fp[1][pick]
    va = [xs.point_kernels(np.maximum(ra * (1 + s * h), xs.FLOOR), rb, functional) for s in (1, -1)]
    vb = [xs.point_kernels(ra, np.maximum(rb * (1 + s * h), xs.FLOOR), functional) for s in (1, -1)]
    for row, (k, gk) in enumerate(zip(("f_X_aa", "f_X_bb", "f_C_aa", "f_C_ab", "f_C_bb"), ("fxaa_pick", "fxbb_pick", "fcaa_pick", "fcab_pick", "fcbb_pick")), start=2):
        d = np.abs(fp[row] - pk[k])
        slope_a, slope_b = np.abs(va[0][k] - va[1][k]) / (2 * h * ra), np.abs(vb[0][k] - vb[1][k]) / (2 * h * rb)
        d_stored = np.abs(fp[row][pick] - g[gk])
        allowed = xs.POINT_TOL * pk["mag_" + k][pick] + 1.01 * (slope_a * np.abs(ra - g["rho_a_pick"]) + slope_b * np.abs(rb - g["rho_b_pick"]))
        print(f"[{tag} {k}] max |d| / mag = {np.max(d / np.maximum(pk['mag_' + k], 1e-300)) / EPS:.1f} eps on the grid; against the stored picks "
              f"{np.max(d_stored / np.maximum(allowed, 1e-300)):.2f} of the allowance")
        assert np.all(d <= xs.POINT_TOL * pk["mag_" + k]) and np.all(d_stored <= allowed)


@pytest.mark.parametrize("name,functional", [("HFS", "HFS"), ("VWN5", "SVWN"), ("VWN3", "SVWN3")])
def test_point_kernels_on_the_ladder_and_at_full_polarisation(eng, utddft_golden, name, functional):
    """The ladder of (rho_alpha, rho_beta) pairs -- zeta = 0, |zeta| -> 1, a spin at the floor, both at the floor -- holds the reference's
    values at densities no orbital produces, and the library takes densities from density matrices only.  The chain is closed in two
    links with the same bound, POINT_TOL of the sums of the magnitudes of the terms: the model equals the stored ladder (here and in
    tests/test_xc_kernel_spin_reference.py), and the device equals the model at every density it produces for the ladder's regimes --
    here the H atom (1, 0) with each functional, whose rho_beta sits at the floor on the whole grid (zeta = 1 - 2e-23 / rho where rho
    is live, both floors in the tail); zeta = 0 and every zeta in between are test_point_kernels_against_the_model's."""
    lad = utddft_golden["ladder"][name]
    pk = xs.point_kernels(lad[0], lad[1], functional)
    for row, k in enumerate(("f_X_aa", "f_X_bb", "f_C_aa", "f_C_ab", "f_C_bb"), start=2):
        if (name == "HFS") == k.startswith("f_X"):            # (the ladder of a correlation functional holds no exchange, and the reverse)
            assert np.all(np.abs(pk[k] - lad[row]) <= xs.POINT_TOL * pk["mag_" + k])
    tag = "h_lda_631g"
    g = utddft_golden[tag]
    r = xs.rebuilt(tag)
    eng.set_basis(r["aos"]).build_eri(True)
    eng.dft_setup(r["pts"], r["wts"], functional)
    K, fp = eng.xc_kernel_uhf(g["C_alpha"], g["C_beta"], g["P_alpha"], g["P_beta"], 1, 0, return_points=True)
    assert np.all(fp[1] == xs.FLOOR)                          # rho_beta at the floor on the whole grid
    pm = xs.point_kernels(fp[0], fp[1], functional, floored=True)
    for row, k in enumerate(("f_X_aa", "f_X_bb", "f_C_aa", "f_C_ab", "f_C_bb"), start=2):
        assert np.isfinite(fp[row]).all() and np.all(np.abs(fp[row] - pm[k]) <= xs.POINT_TOL * pm["mag_" + k]), k


@pytest.mark.parametrize("tag", list(xs.SYSTEMS))
def test_kernel_matrices_against_the_stored_ones(eng, utddft_golden, tag):
    """K of every golden system and window, element by element within 2 gamma_G S + RHO_TOL D (xs.k_bound), symmetric to the last bit and
    the same bits in a second call -- on every tensor layout: the kernel build does not read the tensor."""
    g = utddft_golden[tag]
    na, nb = int(g["n_alpha"]), int(g["n_beta"])
    models = {k: xs.golden_model(tag, g, k) for k in xs.frozen_variants(g)}
    first = {}
    for layout in ("packed", "rows", "tiles"):
        usetup(eng, tag, layout=layout)
        assert eng.eri_storage()["layout"] == layout
        for k, m in models.items():
            K = eng.xc_kernel_uhf(g["C_alpha"], g["C_beta"], g["P_alpha"], g["P_beta"], na, nb, k // 2, k // 2)
            again = eng.xc_kernel_uhf(g["C_alpha"], g["C_beta"], g["P_alpha"], g["P_beta"], na, nb, k // 2, k // 2)
            want, bound = g[f"K_fc{k}"], xs.k_bound(m)
            d = np.abs(K - want)
            print(f"\n[{tag} {layout} fc{k}] dim {len(want)} max |dK| {d.max():.1e} max |dK| / bound {np.max(d / np.maximum(bound, 1e-300)):.1e} "
                  f"(largest bound {bound.max():.1e})")
            assert np.all(d <= bound) and np.array_equal(K, K.T) and np.array_equal(K, again)
            assert np.array_equal(K, first.setdefault(k, K)), layout


@pytest.mark.parametrize("tag", list(xs.SYSTEMS))
def test_states_and_stability_against_the_goldens(eng, utddft_golden, tag):
    """Every TDA and TD-DFT energy of the stable systems, |mu| and f as sums over clusters of degenerate states, all-electron and with a
    frozen orbital per spin; the lowest Hessian eigenvalue of every system.  The two unstable systems (xs.UNSTABLE: LiH at 4.0 and H2 at
    3.0 angstrom on the restricted solution past the spin-symmetry breaking point, Hessian eigenvalues -0.078 and -0.146) are stored with
    their markers only: their verdict is reproduced as a RESULT of tf_stability_uks -- the negative eigenvalue within the same bound --
    and full TD-DFT refuses them with TF_ELINALG where the reference drops roots.  Allowed for energies and eigenvalues: CIS_TOL, TDHF_TOL
    and STAB_TOL of the Hartree-Fock tests plus ||dK||, the Frobenius norm of the element-wise bound of the kernel matrix, by which an
    eigenvalue of a symmetric matrix can move (twice for A + B, which carries 2 K); for the cluster sums of |mu| and f MOMENT_TOL of the
    Hartree-Fock tests as it stands (its derivation, a perturbation of 1e-11 over the smallest gap, covers ||dK|| <= 4e-11 here)."""
    g = utddft_golden[tag]
    usetup(eng, tag)
    Ca, Cb, ea, eb = spin_orbitals(g)
    na, nb = int(g["n_alpha"]), int(g["n_beta"])
    bad = []
    for k in xs.frozen_variants(g):
        dK = np.linalg.norm(xs.k_bound(xs.golden_model(tag, g, k)))
        s = eng.stability_uks(Ca, Cb, ea, eb, g["P_alpha"], g["P_beta"], na, nb, k // 2, k // 2)
        want = float(g[f"stab_fc{k}_lowest"])
        print(f"\n[{tag} fc{k}] lowest Hessian eigenvalue {s['lowest']:.10f} from {s['source']} (golden {want:.10f}, d {abs(s['lowest'] - want):.1e}, tol {STAB_TOL + 2 * dK:.1e})")
        assert abs(s["lowest"] - want) <= STAB_TOL + 2 * dK and (s["lowest"] > -1e-5) == (want > -1e-5)
        assert (tag in xs.UNSTABLE) == (want <= -1e-5) == (f"TDDFT_fc{k}_unstable" in g)
        if not xs.stable(g, k):
            assert tag in xs.UNSTABLE and s["source"] == "plus"                               # a spin-symmetry breaking rotation: A + B
            with pytest.raises(TunaError, match="unstable") as e:
                eng.tddft_uhf(Ca, Cb, ea, eb, g["P_alpha"], g["P_beta"], na, nb, k // 2, k // 2, method="TDDFT")
            assert e.value.code == -5
            tda = eng.tddft_uhf(Ca, Cb, ea, eb, g["P_alpha"], g["P_beta"], na, nb, k // 2, k // 2, method="TDA")
            assert tda["dim"] == s["dim"] and np.isfinite(tda["E"]).all()                    # TDA needs no positive definite Hessian
            continue
        for method, base in (("TDA", CIS_TOL), ("TDDFT", TDHF_TOL)):
            pre = f"{method}_fc{k}_"
            r = eng.tddft_uhf(Ca, Cb, ea, eb, g["P_alpha"], g["P_beta"], na, nb, k // 2, k // 2, method=method, dip=g["dip"])
            ge = g[pre + "energies"]
            tol = base + 2 * dK
            d = np.abs(r["E"] - ge).max()
            mu = np.linalg.norm(r["tdm"], axis=1)
            d_mu = np.abs(cluster_sums(ge, mu) - cluster_sums(ge, g[pre + "tdm"])).max()
            d_f = np.abs(cluster_sums(ge, r["osc"]) - cluster_sums(ge, g[pre + "osc"])).max()
            print(f"[{tag} {method} fc{k}] dim {r['dim']} (alpha {r['dim_alpha']}) max |dE| {d:.1e} (tol {tol:.1e}, of which ||dK|| {dK:.1e}) "
                  f"cluster |mu| d {d_mu:.1e} f d {d_f:.1e} seconds {r['seconds']}")
            assert r["dim"] == len(ge)                                                      # no state is left out
            if not (d <= tol and d_mu <= MOMENT_TOL and d_f <= MOMENT_TOL):
                bad.append((method, k, d, d_mu, d_f))
    assert not bad, bad


@pytest.mark.parametrize("tag", list(xk.SYSTEMS))
def test_restricted_kohn_sham_stability_against_the_goldens(eng, tddft_golden, utddft_golden, tag):
    g = tddft_golden[tag]
    setup(eng, tag)
    m = xk.model_kernel(tag, g, 0)
    g2 = 2 * xk.gamma(m["G"])
    dK = np.linalg.norm(g2 * m["SS"] + xk.RHO_TOL * m["DS"]) + np.linalg.norm(g2 * m["ST"] + xk.RHO_TOL * m["DT"])
    s = eng.stability_rks(g["C"], g["eps"], g["P"], int(g["n_occ"]))
    for mult in ("singlet", "triplet"):
        want = float(utddft_golden["rks"][f"{tag}__{mult}"])
        d = abs(s[f"lowest_{mult}"] - want)
        print(f"\n[{tag} {mult}] lowest {s[f'lowest_{mult}']:.10f} from {s[f'source_{mult}']} (golden d {d:.1e}, tol {STAB_TOL + 2 * dK:.1e})")
        assert d <= STAB_TOL + 2 * dK


def test_calculate_energy_routes_and_prints_the_golden_blocks(eng, utddft_golden):
    """NH / STO-3G UHFS through calculate_energy with a Calculation (the README's snippet, with excited_state and stability_analysis set: the
    input lines themselves stay refused): the unrestricted Kohn-Sham SCF on the golden's grid and thresholds, then
    run_kohn_sham_stability and run_unrestricted_tddft.  out.stability and out.excited are filled, the energies are the golden's within
    the 1e-8 Eh of the project's input-line tests, the stability block is the reference's character for character and the spectrum
    table the reference's row by row (rows of a degenerate cluster compared without their state numbers)."""
    import json
    import os
    from conftest import GOLD
    from test_gpu_cis import same_table, spectrum_rows
    import cis_reference as cr
    from tuna_amd import energy
    with open(os.path.join(GOLD, "utddft_text.json")) as f:
        texts = json.load(f)
    g = utddft_golden["nh_hfs_sto3g"]
    _, _, basis, symbols, R, params = energy.parse_input("SPE : N H 1.036 : HFS STO-3G : ML 3 EXTREME LOOSEGRID NSTATES 5")
    calc = energy.interpret_keywords(params, energy.Calculation("SPE", "HFS", basis))
    calc.functional, calc.reference = "HFS", "UHF"            # (the README's snippet: what run() builds for the UHFS line, without its refusals)
    captured = {"symbols": symbols, "R": R, "calc": calc}
    for t in (t for t in texts if t["kind"] == "excited"):
        calc = captured["calc"]
        calc.stability_analysis, calc.excited_state, calc.tamm_dancoff_approximation = True, "TD-HFS", t["method"] == "TDA"
        log = []
        out = energy.calculate_energy(captured["symbols"], captured["R"], calc, eng, False, log.append)
        want = g[t["prefix"] + "energies"]
        E_SCF = float(g["E_SCF"])
        print(f"\n[{t['method']}] E = {out.energy:.10f} (golden {E_SCF + want[0]:.10f}, d {out.energy - E_SCF - want[0]:.1e}) lowest Hessian eigenvalue "
              f"{out.stability['lowest']:.8f} (golden {float(g['stab_fc0_lowest']):.8f}) seconds {out.excited['seconds']}")
        assert abs(out.energy - (E_SCF + want[0])) < 1e-8 and np.abs(out.excited["energies"] - want).max() < 1e-8
        assert abs(out.stability["lowest"] - float(g["stab_fc0_lowest"])) < 1e-8 and out.stability["stable"] and out.stability["reference"] == "UHF"
        assert out.excited["method"] == "TD-HFS" and out.excited["dim"] == len(want)
        text = "\n".join(log).split("\n")
        stab = next(x for x in texts if x["kind"] == "stability" and x["reference"] == "UHF")["text"].strip("\n").split("\n")
        k = next(n for n, s in enumerate(text) if "Stability Analysis" in s)
        assert text[k - 1:k - 1 + len(stab)] == stab
        joined = "\n".join(text)
        for s in (" Evaluating exchange-correlation kernel...   [Done]", "      Time-dependent Density Functional Theory", "Final single point energy:",
                  ("  Using" if t["method"] == "TDA" else "  Not using") + " the Tamm-Dancoff approximation..."):
            assert s in joined, s
        assert joined.count(" Evaluating molecular orbitals on grid...    [Done]") == 2       # the stability analysis and the excited states
        rows, ref_rows = spectrum_rows(log), spectrum_rows(t["text"].split("\n"))
        assert len(rows) == len(ref_rows) == 5
        for c in cr.clusters(want[:5]):
            same_table(sorted(rows[n][-5:] for n in c), sorted(ref_rows[n][-5:] for n in c))
