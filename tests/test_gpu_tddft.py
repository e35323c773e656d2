"""GPU: closed-shell TD-DFT and TDA for the local-density functionals -- the point kernels (tfdft::xc_fpoint_kernel), the kernel
matrices (tf_xc_kernel_rhf: psi GEMM, tfxck::xck_kernel, the slab sum), the driver (tf_tddft_rhf: the shared assembly and solve stages of
tf_cis_rhf) and the input lines -- against the reference program's own numbers (tests/golden/tddft_systems.npz, tddft_text.json), the
NumPy model of tests/xc_kernel_reference.py, and, independent of both, the linear response of V_XC.  Every test that sets a grid clears
it and hands the shared context back with the default layout.

Measured on one MI355X (the prints of these tests): f_X, f_C^S, f_C^T within 3.0 eps of the sum of the magnitudes of their terms of
the model at the device's own density; the density within 1.4e-14 of the sum of the magnitudes of ITS terms of the model's and within
9.3e-14 of the reference's; K_S, K_T within 2.8e-15 of the stored matrices (1.9e-3 of the bound), the same bits on the three layouts;
TDA energies within 3.2e-14 Eh, TD-DFT energies within 2.8e-13 Eh, cluster sums of |mu| within 4.6e-13 and of f within 1.7e-13; the
linear-response identity within 5.1e-8 (singlet) and 2.7e-8 (triplet) of 2 K kappa, whose largest elements are 0.10 and 0.088, at
h = 5e-4, against its own estimate of the stencil error 1.5e-7 and 8.2e-8; the two input lines within 9.3e-13 Eh of the golden energy."""
import json
import os

import numpy as np
import pytest

import cis_reference as cr
import xc_kernel_reference as xk
from conftest import GOLD
from test_cis_reference import CIS_TOL, MOMENT_TOL, TDHF_TOL, cluster_sums
from test_cis_reference import split as cis_split
from test_cis_reference import system as cis_system
from test_gpu_cis import same_table, spectrum_rows
from test_gpu_mp3 import _reset
from tuna_amd import energy
from tuna_amd._lib import TunaError

pytestmark = pytest.mark.gpu

TF_EINVAL = -1
POINT_TOL = 64 * xk.EPS


@pytest.fixture(scope="module")
def tddft_golden(golden):
    return xk.split(golden("tddft_systems"))


@pytest.fixture
def eng(engine):
    """the shared context; whatever the test leaves, the grid is cleared and the layout is the default again"""
    yield engine
    engine.dft_clear()
    _reset(engine)


def setup(engine, tag, functional="golden", layout=None):
    r = xk.rebuilt(tag)
    engine.set_basis(r["aos"]).build_eri(True, layout=layout)
    engine.dft_setup(r["pts"], r["wts"], xk.SYSTEMS[tag][4] if functional == "golden" else functional)
    return r


def k_bounds(m):
    """per element: two float64 sums of G terms in any order, plus what a density within RHO_TOL of the sum of its terms' magnitudes moves"""
    g2 = 2 * xk.gamma(m["G"])
    return g2 * m["SS"] + xk.RHO_TOL * m["DS"], g2 * m["ST"] + xk.RHO_TOL * m["DT"]


@pytest.mark.parametrize("tag", list(xk.SYSTEMS))
def test_point_kernels_at_the_picked_points(eng, tddft_golden, tag):
    """f_points of the golden systems at the 400 picked points.  The density first: within RHO_TOL of the sum of the magnitudes of its
    terms of the reference's -- a failure of its own.  Then each kernel against the model AT THE DEVICE'S density, f_X within 64 eps of
    itself and the VWN terms within 64 eps of the sum of the magnitudes of the terms of their closed forms: the logarithm and arctangent
    terms of a VWN fit cancel (to 1e-6 of their magnitudes at rho = 1e3, test_xc_kernel_reference), so a result computed in another
    order of operations differs by roundings of that sum, not of the value.  And against the STORED values with the first-order effect
    of the two densities' difference added, |df/drho| |rho - rho_ref|."""
    g = tddft_golden[tag]
    functional = xk.SYSTEMS[tag][4]
    setup(eng, tag)
    m = xk.model_kernel(tag, g)
    KS, KT, fp = eng.xc_kernel_rhf(g["C"], g["P"], int(g["n_occ"]), 0, return_points=True)
    pick = g["pick"]
    assert fp.shape == (4, m["G"]) and np.isfinite(fp).all() and fp[0].min() == xk.FLOOR
    d_rho = np.abs(fp[0] - m["rho"]) / m["rho_mag"]
    d_ref = np.abs(fp[0][pick] - g["rho_pick"]) / m["rho_mag"][pick]
    print(f"\n[{tag}] G {m['G']} max |rho - model| / rho_mag {d_rho.max():.1e}, |rho - reference| / rho_mag at the picks {d_ref.max():.1e} (tol {xk.RHO_TOL:.0e})")
    assert d_rho.max() <= xk.RHO_TOL and d_ref.max() <= xk.RHO_TOL
    pk = xk.point_kernels(fp[0], functional)                  # the model at the device's own (floored) density, every point of the grid
    h = 1e-6
    up, dn = xk.point_kernels(fp[0] * (1 + h), functional), xk.point_kernels(fp[0] * (1 - h), functional)
    for row, (k, mk, gk) in enumerate((("f_X", "mag_X", "fx_pick"), ("f_CS", "mag_CS", "fcs_pick"), ("f_CT", "mag_CT", "fct_pick")), start=1):
        d = np.abs(fp[row] - pk[k])
        slope = np.abs(up[k] - dn[k]) / (2 * h * fp[0])       # |df / drho|
        d_stored = np.abs(fp[row][pick] - g[gk])
        allowed = POINT_TOL * pk[mk][pick] + 1.01 * slope[pick] * np.abs(fp[0][pick] - g["rho_pick"])
        print(f"[{tag} {k}] max |d| / mag = {np.max(d / np.maximum(pk[mk], 1e-300)) / xk.EPS:.1f} eps on the grid; against the stored picks "
              f"{np.max(d_stored / np.maximum(allowed, 1e-300)):.2f} of the allowance")
        assert np.all(d <= POINT_TOL * pk[mk]) and np.all(d_stored <= allowed)
    if functional == "HFS":
        assert not fp[2].any() and not fp[3].any() and np.array_equal(KS, KT)


@pytest.mark.parametrize("tag", list(xk.SYSTEMS))
def test_kernel_matrices_against_the_stored_ones(eng, tddft_golden, tag):
    """K_S and K_T of every golden system, all-electron and with a frozen orbital, element by element within 2 gamma_G S + RHO_TOL D
    (k_bounds), symmetric to the last bit and the same bits in a second call -- on every tensor layout: the kernel build does not read
    the tensor, so the layouts must give the same bits."""
    g = tddft_golden[tag]
    nocc = int(g["n_occ"])
    models = {nf: xk.model_kernel(tag, g, nf) for nf in xk.frozen_variants(g)}
    packed = {}
    for layout in ("packed", "rows", "tiles"):
        setup(eng, tag, layout=layout)
        assert eng.eri_storage()["layout"] == layout
        for nf, m in models.items():
            K = eng.xc_kernel_rhf(g["C"], g["P"], nocc, nf)
            again = eng.xc_kernel_rhf(g["C"], g["P"], nocc, nf)
            for mult, got, rep, bound in zip(("singlet", "triplet"), K, again, k_bounds(m)):
                want = g[f"K_fc{nf}_{mult}"]
                d = np.abs(got - want)
                print(f"\n[{tag} {layout} fc{nf} {mult}] dim {len(want)} max |dK| {d.max():.1e} max |dK| / bound {np.max(d / bound):.1e} "
                      f"(largest bound {bound.max():.1e})")
                assert np.all(d <= bound) and np.array_equal(got, got.T) and np.array_equal(got, rep)
            ref = packed.setdefault(nf, K)
            assert all(np.array_equal(x, y) for x, y in zip(K, ref)), layout


def test_linear_response_identity(eng, tddft_golden):
    """Independent of the reference and of the model: K kappa against the central difference of V_XC on CO / 6-31G LDA.

    Closed shell, P = 2 C_o C_o^T.  Rotating the occupied orbitals by kappa [o, v], C_o -> C_o + C_v kappa^T, changes the density
    matrix by dP = 2 (C_v kappa^T C_o^T + C_o kappa C_v^T) to first order and the density by dn = 4 sum_jb kappa_jb psi_j psi_b.  With
    F(n) = n e_xc(n), V_XC = int w F'(n) phi phi, so d/dh V_XC[P + h dP] = int w F''(n) dn phi phi, and between an occupied and a
    virtual orbital
        [C_o^T (dV/dh) C_v]_ia = sum_g w F'' psi_i psi_a 4 sum_jb kappa_jb psi_j psi_b = 2 (K_S kappa)_ia,
    because u_S = w 2 F'' (f_X = 2 d2(n e_X)/dn2, f_C^S likewise).  For the triplet, rotate the alpha orbitals by kappa and the beta
    orbitals by -kappa: dP_alpha = -dP_beta = dP / 2, dn_alpha = -dn_beta = 2 sum kappa psi psi, and
        dV_alpha = int w (f_aa dn_alpha + f_ab dn_beta) phi phi = int w (f_aa - f_ab) dn_alpha phi phi,  f_aa - f_ab = u_T / w
    (exchange: f_aa = 2 F_x'', f_ab = 0; correlation: 2 f_mm), so [C_o^T (dV_alpha/dh) C_v]_ia = 2 (K_T kappa)_ia as well.
    A kernel without its factor of 2 misses by |K kappa| itself.

    The tolerance is the stencil's own error: D(h) = exact + c h^2 + ..., so D(h) - D(h / 2) = 3/4 c h^2 is three times the error of
    D(h / 2); the largest |D(h) - D(h / 2)| over the elements bounds it with that factor to spare, plus the rounding of the difference
    quotient, 8 eps max |V| / h."""
    tag = "co_lda_631g"
    g = tddft_golden[tag]
    setup(eng, tag)
    nocc = 7
    C = g["C"]
    Co, Cv = C[:, :nocc], C[:, nocc:]
    KS, KT = eng.xc_kernel_rhf(C, g["P"], nocc, 0)
    kappa = np.random.default_rng(11).standard_normal((nocc, Cv.shape[1]))
    kappa /= np.abs(kappa).max()
    dP = 2 * (Cv @ kappa.T @ Co.T + Co @ kappa @ Cv.T)
    P = g["P"]
    v_max = np.abs(eng.dft_vxc(P)[0]).max()

    def quotient(h):
        s = (eng.dft_vxc(P + h * dP)[0] - eng.dft_vxc(P - h * dP)[0]) / (2 * h)
        ua, ub = eng.dft_vxc_unrestricted(P / 2 + h * dP / 2, P / 2 - h * dP / 2), eng.dft_vxc_unrestricted(P / 2 - h * dP / 2, P / 2 + h * dP / 2)
        t = (ua[0] - ub[0]) / (2 * h)
        return Co.T @ s @ Cv, Co.T @ t @ Cv
    h = 1e-3
    coarse, fine = quotient(h), quotient(h / 2)
    for mult, K, Dh, Dh2 in (("singlet", KS, coarse[0], fine[0]), ("triplet", KT, coarse[1], fine[1])):
        want = 2 * (K @ kappa.ravel()).reshape(kappa.shape)
        stencil = np.abs(Dh - Dh2).max()
        tol = stencil + 8 * xk.EPS * v_max / (h / 2)
        d = np.abs(Dh2 - want).max()
        print(f"\n[{mult}] max |2 K kappa| {np.abs(want).max():.3e} max |D(h/2) - 2 K kappa| {d:.1e} stencil estimate |D(h) - D(h/2)| {stencil:.1e} tol {tol:.1e}")
        assert d <= tol and tol < 1e-4 * np.abs(want).max()
        assert np.abs(Dh2 - 0.5 * want).max() > 100 * tol                                  # a factor of 2 would show


def merged(r):
    return energy.merge_excited_states(r["E_singlet"], r["E_triplet"], r["tdm"], r["osc"])


@pytest.mark.parametrize("tag", list(xk.SYSTEMS))
def test_states_against_the_goldens(eng, tddft_golden, tag):
    """Every TDA and TD-DFT energy of both multiplicities, |mu| and f as sums over clusters of degenerate states, all-electron and with a
    frozen orbital.  The deviation allowed is that of test_gpu_cis.py for the same quantities (CIS_TOL, TDHF_TOL, MOMENT_TOL) plus
    ||dK||, the Frobenius norm of the element-wise bound of the kernel matrices (k_bounds): an eigenvalue of a symmetric matrix moves by
    no more than the norm of the perturbation."""
    g = tddft_golden[tag]
    setup(eng, tag)
    nocc = int(g["n_occ"])
    bad = []
    for nf in xk.frozen_variants(g):
        dK = max(np.linalg.norm(b) for b in k_bounds(xk.model_kernel(tag, g, nf)))
        for method, base in (("TDA", CIS_TOL), ("TDDFT", TDHF_TOL)):
            pre = f"{method}_fc{nf}_"
            r = eng.tddft_rhf(g["C"], g["eps"], g["P"], nocc, nf, method=method, dip=g["dip"])
            tol = base + dK
            d = [np.abs(r[f"E_{m}"] - g[pre + f"E_{m}"]).max() for m in ("singlet", "triplet")]
            e, lab, _, mu, f = merged(r)
            ge = g[pre + "energies"]
            d_mu = np.abs(cluster_sums(ge, mu) - cluster_sums(ge, g[pre + "tdm"])).max()
            d_f = np.abs(cluster_sums(ge, f) - cluster_sums(ge, g[pre + "osc"])).max()
            print(f"\n[{tag} {method} fc{nf}] dim {r['dim']} max |dE| singlet {d[0]:.1e} triplet {d[1]:.1e} (tol {tol:.1e}, of which ||dK|| {dK:.1e}) "
                  f"cluster |mu| d {d_mu:.1e} f d {d_f:.1e} seconds {r['seconds']}")
            assert r["dim"] == len(g[pre + "E_singlet"]) and np.abs(e - ge).max() <= max(d) + 1e-300
            assert np.all(mu[lab == "triplet"] == 0) and np.all(f[lab == "triplet"] == 0)
            if not (max(d) <= tol and d_mu <= MOMENT_TOL + dK and d_f <= MOMENT_TOL + dK):
                bad.append((method, nf, d, d_mu, d_f))
    assert not bad, bad


def test_null_functional_is_cis_and_tdhf_bit_for_bit(eng, golden):
    """tf_dft_setup with exchange and correlation ids 0 and hfx = 1: no kernel is built, the exchange blocks are multiplied by 1.0,
    and every output of tddft_rhf -- energies, vectors, moments, the assembled matrices -- is cis_rhf's, CIS and TDHF, to the last bit."""
    g = cis_split(golden("cis_systems"))["co_631g"]
    aos = cis_system("co_631g")[1]
    r = xk.rebuilt("co_lda_631g")
    eng.set_basis(aos).build_eri(True)
    f = eng.dft_setup(r["pts"], r["wts"], None)
    assert f["hfx"] == 1.0 and f["name"] == "NONE"
    nocc = int(g["n_occ"])
    P = 2 * g["C"][:, :nocc] @ g["C"][:, :nocc].T
    for nf in (0, 1):
        for cis_name, td_name in (("CIS", "TDA"), ("TDHF", "TDDFT")):
            a = eng.cis_rhf(g["C"], g["eps"], nocc, nf, method=cis_name, n_keep=5, dip=g["dip"], return_matrices=True)
            b = eng.tddft_rhf(g["C"], g["eps"], P, nocc, nf, method=td_name, n_keep=5, dip=g["dip"], return_matrices=True)
            assert set(a) == set(b)
            for key in a:
                if key == "seconds":
                    continue
                if a[key] is None:
                    assert b[key] is None, key
                else:
                    assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (cis_name, nf, key)
    KS, KT = eng.xc_kernel_rhf(g["C"], P, nocc, 0)            # the kernel of nothing is nothing
    assert not KS.any() and not KT.any()


def test_half_exact_exchange_assembly(eng, golden):
    """Null functional, hfx = 0.5: the returned matrices against a NumPy assembly from ao_to_mo's blocks,
    A + B singlet = Delta + 4 G - hfx (H + X), triplet = Delta - hfx (H + X), A - B = Delta - hfx (H - X); CIS: A = Delta + 2 G - hfx H,
    Delta - hfx H; within 1e-11 of the largest entry (test_gpu_cis.py's bar for the same matrices).  And hfx = 0: (ab|ij) is not built;
    A - B is the diagonal of orbital-energy differences exactly."""
    g = cis_split(golden("cis_systems"))["co_631g"]
    aos = cis_system("co_631g")[1]
    r = xk.rebuilt("co_lda_631g")
    eng.set_basis(aos).build_eri(True)
    eng.dft_setup(r["pts"], r["wts"], None)
    nocc, nf = int(g["n_occ"]), 1
    C, eps = g["C"], g["eps"]
    Co, Cv = C[:, nf:nocc], C[:, nocc:]
    o, v = Co.shape[1], Cv.shape[1]
    dim = o * v
    ovov = eng.ao_to_mo(Co, Cv, Co, Cv)
    G = ovov.reshape(dim, dim)
    X = ovov.transpose(0, 3, 2, 1).reshape(dim, dim)
    H = eng.ao_to_mo(Co, Co, Cv, Cv).transpose(0, 2, 1, 3).reshape(dim, dim)
    D = np.diag((eps[nocc:][None, :] - eps[nf:nocc][:, None]).ravel())
    P = 2 * C[:, :nocc] @ C[:, :nocc].T
    sym = cr._sym
    for hfx in (0.5, 0.0):
        want = {"TDDFT": {"M_plus_singlet": sym(D + 4 * G - hfx * (H + X)), "M_plus_triplet": sym(D - hfx * (H + X)), "M_minus": sym(D - hfx * (H - X))},
                "TDA": {"M_plus_singlet": sym(D + 2 * G - hfx * H), "M_plus_triplet": sym(D - hfx * H)}}
        for method, mats in want.items():
            got = eng.tddft_rhf(C, eps, P, nocc, nf, method=method, hfx=hfx, return_matrices=True)
            for key, M in mats.items():
                d = np.abs(got[key] - M).max() / np.abs(M).max()
                print(f"\n[hfx {hfx} {method} {key}] max |d| / max |entry| {d:.1e}")
                assert d <= 1e-11 and np.array_equal(got[key], got[key].T)
            if method == "TDA":
                assert got["M_minus"] is None
            elif hfx == 0.0:
                assert np.array_equal(got["M_minus"], D)
            assert np.abs(got["E_singlet"] - (cr.cis(mats["M_plus_singlet"])[0] if method == "TDA" else
                                              cr.tdhf_cholesky(mats["M_plus_singlet"], mats["M_minus"])["E"])).max() < CIS_TOL


def test_refusals(eng, tddft_golden):
    tag = "hf_svwn_631g"
    g = tddft_golden[tag]
    r = setup(eng, tag)
    nocc = int(g["n_occ"])
    first = eng.tddft_rhf(g["C"], g["eps"], g["P"], nocc, 0, method="TDA")

    def still_usable():
        again = eng.tddft_rhf(g["C"], g["eps"], g["P"], nocc, 0, method="TDA")
        assert np.array_equal(again["E_singlet"], first["E_singlet"]) and np.array_equal(again["E_triplet"], first["E_triplet"])
    for call in (lambda: eng.tddft_rhf(g["C"], g["eps"], None, nocc, 0), lambda: eng.xc_kernel_rhf(g["C"], None, nocc, 0),
                 lambda: eng.tddft_rhf(g["C"], g["eps"], g["P"], nocc, nocc), lambda: eng.tddft_rhf(g["C"], g["eps"], g["P"], len(g["eps"]), 0),
                 lambda: eng.tddft_rhf(g["C"], g["eps"], g["P"], nocc, 0, singlets=False, triplets=False),
                 lambda: eng.tddft_rhf(g["C"], g["eps"], g["P"], nocc, 0, hfx=float("nan")), lambda: eng.xc_kernel_rhf(g["C"], g["P"], 0, 0)):
        with pytest.raises(TunaError) as e:
            call()
        assert e.value.code == TF_EINVAL and ("tf_tddft_rhf" in str(e.value) or "tf_xc_kernel_rhf" in str(e.value))
        still_usable()
    # a gradient-corrected functional: the message names it
    for functional, names in (("BLYP", ("B88", "LYP")), ("B3LYP", ("B3", "3P")), ("SLYP", ("Slater", "LYP")), ("HFB", ("B88", "none"))):
        eng.dft_setup(r["pts"], r["wts"], functional)
        for call in (lambda: eng.tddft_rhf(g["C"], g["eps"], g["P"], nocc, 0), lambda: eng.xc_kernel_rhf(g["C"], g["P"], nocc, 0)):
            with pytest.raises(TunaError, match="exchange-correlation kernel") as e:
                call()
            assert e.value.code == TF_EINVAL and all(n in str(e.value) for n in names), str(e.value)
    eng.dft_setup(r["pts"], r["wts"], "SVWN")
    still_usable()
    # without a grid
    eng.dft_clear()
    for call in (lambda: eng.tddft_rhf(g["C"], g["eps"], g["P"], nocc, 0), lambda: eng.xc_kernel_rhf(g["C"], g["P"], nocc, 0)):
        with pytest.raises(TunaError, match="tf_dft_setup") as e:
            call()
        assert e.value.code == TF_EINVAL
    ok = eng.cis_rhf(g["C"], g["eps"], nocc, 0, method="CIS")                              # the context stays usable
    assert ok["dim"] == first["dim"]
    from tuna_amd.engine import Engine
    with Engine(0) as fresh:                                                                # no tensor yet
        from tuna_amd._lib import f64, ptr
        fresh.set_basis(r["aos"])
        Cc, Pc, K = f64(g["C"]), f64(g["P"]), np.zeros((first["dim"], first["dim"]))
        assert fresh._L.tf_xc_kernel_rhf(fresh._ctx, nocc, 0, ptr(Cc), ptr(Pc), ptr(K), ptr(K), None) == TF_EINVAL
        assert "tf_build_eri" in fresh._L.tf_last_error(fresh._ctx).decode()


def test_input_lines(eng, tddft_golden):
    """`SPE : C O 1.128 : SVWN 6-31G : TD NSTATES 5` and its TD TDA variant on the golden's grid (LOOSEGRID) and thresholds (EXTREME):
    out.energy = E_SCF + w_root within the 1e-8 Eh of the project's input-line tests, every merged energy within 1e-8, and the printed
    spectrum against what the reference prints (rows of a degenerate cluster compared without their state numbers)."""
    from tuna_amd.energy import run
    with open(os.path.join(GOLD, "tddft_text.json")) as f:
        texts = {t["line"]: t for t in json.load(f)}
    g = tddft_golden["co_lda_631g"]
    E_SCF = float(g["E_SCF"])
    for line, key, pre, root in (("SPE : C O 1.128 : SVWN 6-31G : EXTREME LOOSEGRID TD NSTATES 5", "SPE : C O 1.128 : SVWN 6-31G : TD NSTATES 5", "TDDFT_fc0_", 1),
                                 ("SPE : C O 1.128 : SVWN 6-31G : EXTREME LOOSEGRID TD TDA NSTATES 5 ROOT 3", "SPE : C O 1.128 : SVWN 6-31G : TD TDA NSTATES 5", "TDA_fc0_", 3)):
        log = []
        out = run(line, silent=False, engine=eng, log=log.append)
        want = g[pre + "energies"]
        print(f"\n[{line}] E = {out.energy:.10f} (golden {E_SCF + want[root - 1]:.10f}, d {out.energy - E_SCF - want[root - 1]:.1e}) seconds {out.excited['seconds']}")
        assert abs(out.energy - (E_SCF + want[root - 1])) < 1e-8 and np.abs(out.excited["energies"] - want).max() < 1e-8
        assert out.excited["method"] == "TD-SVWN" and out.excited["root"] == root
        d_f = np.abs(cluster_sums(want, out.excited["oscillator_strengths"]) - cluster_sums(want, g[pre + "osc"])).max()
        assert d_f < MOMENT_TOL
        text = "\n".join(log)
        for s in (" Evaluating molecular orbitals on grid...    [Done]", " Evaluating exchange-correlation kernel...   [Done]",
                  " Calculating matrix elements...              [Done]", "      Time-dependent Density Functional Theory",
                  f"Excitation energy is the energy difference to excited state {root}.", "Final single point energy:"):
            assert s in text, s
        assert f" Excitation energy from {'TD-SVWN:':<11} {out.excited['E_transition']:15.10f}" in text
        assert ("  Using the Tamm-Dancoff approximation..." in text) == ("TDA" in line)
        ref = texts[key]["text"].split("\n")
        rows, ref_rows = spectrum_rows(log), spectrum_rows(ref)
        assert [r[:5] for r in rows] == [r[:5] for r in ref_rows] and len(rows) == 5
        for c in cr.clusters(want[:len(ref_rows)]):
            same_table(sorted(rows[n][5:] for n in c), sorted(ref_rows[n][5:] for n in c))
    for line in ("SPE : C O 1.128 : B3LYP 6-31G : TD", "SPE : C O 1.128 : BLYP 6-31G : TD TDA", "SPE : C O 1.128 : SVWN 6-31G : TD (D)",
                 "SPE : C O 1.128 : LDA 6-31G : TD STAB", "SPE : C O 1.128 : TDDFT 6-31G"):
        with pytest.raises(TunaError):
            run(line, engine=eng)
    with pytest.raises(TunaError, match="HF or RHF line only"):
        run("SPE : C O 1.128 : B3LYP 6-31G : TD", engine=eng)
