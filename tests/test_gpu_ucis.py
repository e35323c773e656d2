"""GPU: unrestricted CIS / TDHF and the SCF stability analysis on the resident tensor (tf_cis_uhf, tf_stability_rhf, tf_stability_uhf:
the spin-blocked assembly kernel tfucis::uassemble_kernel and the solve stages shared with tf_cis_rhf) against the reference program's
own numbers (tests/golden/ucis_systems.npz, stability_text.json) and the independent NumPy checker of tests/ucis_reference.py: every
energy of every stored system, transition moments by clusters of degenerate states, the assembled matrices and the kept vectors element
by element at the spin boundary's edge cases, the identity with the restricted routine, the Hessian spectra, the layouts, the refusals
and the STAB input lines.  Every test hands the shared context back with the default layout."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import cis_reference as cr
import ucis_reference as ur
from conftest import GOLD, R_H2
from test_cis_reference import CIS_TOL, MOMENT_TOL, R_H2_UNSTABLE, TDHF_TOL, cluster_sums, split
from test_cis_reference import system as closed_system
from test_gpu_cis import VECTOR_TOL, same_table, up_to_sign
from test_gpu_mp3 import _reset
from test_ucis_reference import (MARGINAL, RANDOM_CASES, RSTAB, STAB_TOL, SYSTEMS, UNSTABLE, UTDHF_TOL, orbitals, random_uhf_orbitals, usystem,
                                 variants, windows)
from tuna_amd import energy
from tuna_amd._lib import StabilityResult, TunaError, UcisOpts, UcisResult, ptr

pytestmark = pytest.mark.gpu

TF_EINVAL, TF_ELINALG = -1, -5


@pytest.fixture(scope="module")
def ucis_golden(golden):
    return split(golden("ucis_systems"))


@pytest.fixture(scope="module")
def cis_golden(golden):
    return split(golden("cis_systems"))


@pytest.fixture(scope="module")
def n2_tz():
    shells, aos = closed_system("n2_ccpvtz")
    return aos, cr.dense_eri(aos, shells)


@pytest.mark.parametrize("tag", list(SYSTEMS))
def test_reference_orbitals_against_goldens(engine, ucis_golden, tag):
    """Every CIS and TDHF energy of every stored system, frozen variants included (CIS within 1e-10 Eh, TDHF within ten times the
    deviation of the CPU checker's Cholesky route from the golden, 2.8e-12 Eh); |mu| and f as sums over clusters of degenerate states; the
    lowest Hessian eigenvalue against the reference's.  O2/STO-3G's UHF solution is a saddle point: TDHF refuses it and CIS returns its
    negative energies.  NO and OH have a zero mode of the Hessian: only their CIS and their Hessian are compared."""
    g = ucis_golden[tag]
    engine.set_basis(usystem(tag)[1]).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed"
    Ca, Cb, ea, eb = orbitals(g)
    bad = []
    for k in variants(tag):
        na, nb, nfa, nfb = windows(g, k)
        for method in ("CIS", "TDHF"):
            pre = f"{method}_fc{k}_"
            if method == "TDHF" and tag in UNSTABLE:
                with pytest.raises(TunaError, match="unstable") as e:
                    engine.cis_uhf(Ca, Cb, ea, eb, na, nb, nfa, nfb, method="TDHF", dip=g["dip"])
                print("\n" + str(e.value))
                assert e.value.code == TF_ELINALG and "UHF reference" in str(e.value)
                continue
            if method == "TDHF" and tag in MARGINAL:
                continue
            r = engine.cis_uhf(Ca, Cb, ea, eb, na, nb, nfa, nfb, method=method, dip=g["dip"])
            tol = CIS_TOL if method == "CIS" else UTDHF_TOL
            ge = g[pre + "energies"]
            d = np.abs(r["E"] - ge).max()
            mu = np.linalg.norm(r["tdm"], axis=1)
            d_mu = np.abs(cluster_sums(ge, mu) - cluster_sums(ge, g[pre + "tdm"])).max()
            d_f = np.abs(cluster_sums(ge, r["osc"]) - cluster_sums(ge, g[pre + "osc"])).max()
            print(f"\n[{tag} {method} fc{k}] dim {r['dim']} (alpha {r['dim_alpha']}) max |dE| {d:.1e} (tol {tol:.1e}) cluster |mu| d {d_mu:.1e} f d {d_f:.1e} "
                  f"seconds {r['seconds']}")
            assert r["dim"] == len(ge) and r["dim_alpha"] == ur.dims(len(ea), na, nb, nfa, nfb)[0]
            assert np.allclose(mu ** 2 * r["E"] * (2 / 3), r["osc"], rtol=1e-12, atol=1e-15)
            if method == "CIS" and tag in UNSTABLE:
                assert r["E"][0] < 0
            if not (d < tol and d_mu < MOMENT_TOL and d_f < MOMENT_TOL):
                bad.append((method, k, d, d_mu, d_f))
        s = engine.stability_uhf(Ca, Cb, ea, eb, na, nb, nfa, nfb)
        d = abs(s["lowest"] - float(g[f"stab_fc{k}_lowest"]))
        print(f"[{tag} fc{k}] lowest Hessian eigenvalue {s['lowest']:.8f} from {s['source']} (golden d {d:.1e})")
        if not d < STAB_TOL:
            bad.append(("stability", k, d))
    assert not bad, bad


@pytest.mark.parametrize("na,nb,nf", RANDOM_CASES)
def test_matrices_and_vectors_against_the_independent_checker(engine, n2_tz, na, nb, nf):
    """N2/cc-pVTZ (N = 60), random orthonormal orbitals of either spin.  (1, 0): d_beta = 0, one partial tile; (2, 1): d_alpha = 116,
    d_beta = 59, the spin boundary inside a tile; (8, 7): d_alpha = 416 = 13 x 32 exactly, d_beta = 371 ragged; (7, 8): more beta than
    alpha; (8, 7) with one frozen orbital per spin.  The assembled matrices element by element within 1e-11 max|entry|, bitwise symmetric,
    the alpha-beta rectangles of A - B exactly 0.0, and bit for bit the same in a second call; the five lowest vectors element by element
    up to a sign per state, X.X - Y.Y = 1 to 1e-12.  The conditions the comparison of vectors needs are asserted from the checker."""
    aos, E = n2_tz
    engine.set_basis(aos).build_eri(True)
    N = engine.N
    Ca, Cb, ea, eb = random_uhf_orbitals(N, na, nb)
    da, db = ur.dims(N, na, nb, nf, nf)
    dim, nk = da + db, 5
    m = ur.matrices(E, Ca, Cb, ea, eb, na, nb, nf, nf)
    ref = ur.tdhf_cholesky(m["plus"], m["minus"])
    assert ref["min_eig_minus"] > 0 and ref["min_w2"] > 0
    bad = []
    for method, names in (("CIS", {"M_plus": "A"}), ("TDHF", {"M_plus": "plus", "M_minus": "minus"})):
        r, again = (engine.cis_uhf(Ca, Cb, ea, eb, na, nb, nf, nf, method=method, n_keep=nk, return_matrices=True) for _ in range(2))
        assert r["dim"] == dim and r["dim_alpha"] == da and (r["M_minus"] is None) == (method == "CIS")
        for key, kind in names.items():
            M, want = r[key], m[kind]
            scale = np.abs(want).max()
            d = np.abs(M - want).max() / scale
            print(f"\n[n_alpha {na} n_beta {nb} frozen {nf} {method} {key}] d_alpha {da} d_beta {db} max|entry| {scale:.2f} max|d| / max|entry| {d:.1e}")
            assert np.array_equal(M, M.T), (method, key)
            assert np.array_equal(M, again[key]), (method, key)
            if kind == "minus":
                assert not M[:da, da:].any() and not M[da:, :da].any()
            if not d <= 1e-11:
                bad.append((method, key, d))
        assert np.array_equal(r["E"], again["E"]) and np.array_equal(r["X"], again["X"]) and np.array_equal(r["Y"], again["Y"])
        X, Y = r["X"], r["Y"]
        k = min(nk, dim)
        assert X.shape == (k, dim)
        if method == "CIS":
            e, V = ur.cis(m["A"])
            wX, wY, tol = V[:, :k].T, np.zeros((k, dim)), CIS_TOL
        else:
            e, wX, wY, tol = ref["E"], ref["X"][:, :k].T, ref["Y"][:, :k].T, 1e-10
        assert k < 2 or np.diff(e[:k + 1]).min() > 1e-6
        dE = np.abs(r["E"] - e).max()
        dX = up_to_sign(X, wX)
        s = np.sign(np.sum(X * wX, axis=1))[:, None]
        dY = np.abs(Y - s * wY).max()
        norm = np.abs(np.sum(X * X - Y * Y, axis=1) - 1).max()
        print(f"[n_alpha {na} n_beta {nb} frozen {nf} {method}] max |dE| {dE:.1e} max |dX| {dX:.1e} max |dY| {dY:.1e} |X.X - Y.Y - 1| {norm:.1e}")
        if method == "CIS":
            assert not Y.any()
        if not (dE < tol and dX < VECTOR_TOL and dY < VECTOR_TOL and norm < 1e-12):
            bad.append((method, dE, dX, dY, norm))
    # the Hessian spectra of the same matrices, every eigenvalue, and the lowest mode
    s, again = (engine.stability_uhf(Ca, Cb, ea, eb, na, nb, nf, nf, return_spectra=True, return_mode=True) for _ in range(2))
    spectra, lowest = ur.hessian_spectra_uhf(m)
    d = max(np.abs(s["spectra"][key] - spectra[key]).max() for key in ("plus", "minus"))
    print(f"[n_alpha {na} n_beta {nb} frozen {nf}] Hessian spectra max |d| {d:.1e} lowest {s['lowest']:.6f} from {s['source']}")
    assert d < STAB_TOL and abs(s["lowest"] - lowest) < STAB_TOL and s["source"] == ("minus" if spectra["minus"][0] < spectra["plus"][0] else "plus")
    assert s["lowest"] == again["lowest"] and all(np.array_equal(s["spectra"][key], again["spectra"][key]) for key in spectra)
    assert abs(np.linalg.norm(s["mode"]) - 1) < 1e-12 and np.abs(m[s["source"]] @ s["mode"] - s["lowest"] * s["mode"]).max() < 1e-9
    assert not bad, bad


@pytest.mark.parametrize("tag", ["co_631g", "hf_ccpvdz"])
def test_identity_with_the_restricted_routine(engine, cis_golden, tag):
    """C_alpha = C_beta = a closed-shell system's RHF orbitals: the unrestricted energies are the merged singlets and triplets of cis_rhf,
    the oscillator strengths agree by clusters, and stability_uhf is min(singlet, triplet) of stability_rhf."""
    g = cis_golden[tag]
    engine.set_basis(closed_system(tag)[1]).build_eri(True)
    C, eps, nocc = g["C"], g["eps"], int(g["n_occ"])
    for method, tol in (("CIS", CIS_TOL), ("TDHF", TDHF_TOL)):
        r = engine.cis_rhf(C, eps, nocc, 0, method=method, dip=g["dip"])
        u = engine.cis_uhf(C, C, eps, eps, nocc, nocc, method=method, dip=g["dip"])
        e, _, _, _, f = energy.merge_excited_states(r["E_singlet"], r["E_triplet"], r["tdm"], r["osc"])
        d, d_f = np.abs(u["E"] - e).max(), np.abs(cluster_sums(e, u["osc"]) - cluster_sums(e, f)).max()
        print(f"\n[{tag} {method}] unrestricted against merged restricted: max |dE| {d:.1e} cluster f d {d_f:.1e}")
        assert u["dim"] == 2 * r["dim"] and d < tol and d_f < MOMENT_TOL
    rs = engine.stability_rhf(C, eps, nocc, return_spectra=True)
    us = engine.stability_uhf(C, C, eps, eps, nocc, nocc)
    assert abs(us["lowest"] - min(rs["lowest_singlet"], rs["lowest_triplet"])) < STAB_TOL


def test_restricted_stability(engine, ucis_golden, cis_golden):
    """tf_stability_rhf: every eigenvalue of the three spectra against the checker, the lowest singlet and triplet eigenvalues against the
    reference's; H2/STO-3G at 2.0 angstrom is singlet stable (A - B = 0.1184) and triplet unstable (A + B = w^2 / (A - B) = -0.3999);
    N2/STO-3G's core-guess orbitals are reported unstable without raising; a second call returns the same bits."""
    rs = ucis_golden["rstab"]
    for tag in RSTAB:
        if tag.startswith("h2_sto3g"):
            aos, E, C, eps = cr.h2_minimal_basis(R_H2_UNSTABLE if tag.endswith("2p0") else R_H2)
            nocc = 1
        elif tag == "n2_ccpvtz":
            continue                                                  # (dim 371: the random-orbital test covers that size)
        else:
            shells, aos = closed_system(tag)
            E = cr.dense_eri(aos, shells)
            C, eps, nocc = cis_golden[tag]["C"], cis_golden[tag]["eps"], int(cis_golden[tag]["n_occ"])
        engine.set_basis(aos).build_eri(True)
        r, again = (engine.stability_rhf(C, eps, nocc, return_spectra=True, return_mode=True) for _ in range(2))
        spectra, ls, lt = ur.hessian_spectra_rhf(E, C, eps, nocc)
        d = max(np.abs(r["spectra"][k] - spectra[k]).max() for k in spectra)
        dg = max(abs(r["lowest_singlet"] - float(rs[f"{tag}__singlet"])), abs(r["lowest_triplet"] - float(rs[f"{tag}__triplet"])))
        print(f"\n[{tag}] lowest singlet {r['lowest_singlet']:.8f} ({r['source_singlet']}) triplet {r['lowest_triplet']:.8f} ({r['source_triplet']}) "
              f"spectra max |d| {d:.1e} golden d {dg:.1e} seconds {r['seconds']}")
        assert d < STAB_TOL and dg < STAB_TOL and abs(r["lowest_singlet"] - ls) < STAB_TOL and abs(r["lowest_triplet"] - lt) < STAB_TOL
        assert r["lowest_singlet"] == again["lowest_singlet"] and all(np.array_equal(r["spectra"][k], again["spectra"][k]) for k in spectra)
        assert abs(np.linalg.norm(r["mode_triplet"]) - 1) < 1e-12
        if tag == "h2_sto3g_2p0":
            assert r["lowest_singlet"] > 0.1 and r["source_singlet"] == "minus" and r["lowest_triplet"] < -0.39 and r["source_triplet"] == "plus_triplet"
        if tag == "n2_sto3g":
            assert r["lowest_singlet"] < -0.4 and r["lowest_triplet"] < -0.4


def test_layouts_agree(engine, ucis_golden):
    tag = "o2_triplet_ccpvdz"
    g = ucis_golden[tag]
    aos = usystem(tag)[1]
    Ca, Cb, ea, eb = orbitals(g)
    na, nb, nfa, nfb = windows(g, 4)
    try:
        for layout in ("packed", "rows", "tiles"):
            engine.set_basis(aos).build_eri(True, layout=layout)
            assert engine.eri_storage()["layout"] == layout
            for method, tol in (("CIS", CIS_TOL), ("TDHF", UTDHF_TOL)):
                r = engine.cis_uhf(Ca, Cb, ea, eb, na, nb, nfa, nfb, method=method, dip=g["dip"])
                d = np.abs(r["E"] - g[f"{method}_fc4_energies"]).max()
                print(f"\n[{method}] {layout} against the golden {d:.1e}")
                assert d < tol and abs(r["osc"].sum() - g[f"{method}_fc4_osc"].sum()) < MOMENT_TOL
            s = engine.stability_uhf(Ca, Cb, ea, eb, na, nb, nfa, nfb)
            assert abs(s["lowest"] - float(g["stab_fc4_lowest"])) < STAB_TOL
    finally:
        _reset(engine)
    engine.set_basis(aos).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed"


def test_refusals(engine, ucis_golden):
    from tuna_amd.engine import Engine
    tag = "li_doublet_631g"
    g = ucis_golden[tag]
    aos = usystem(tag)[1]
    engine.set_basis(aos).build_eri(True)
    na, nb = 2, 1
    first = engine.cis_uhf(*orbitals(g), na, nb, method="TDHF", dip=g["dip"])
    first_stab = engine.stability_uhf(*orbitals(g), na, nb)
    L, ctx, N = engine._L, engine._ctx, engine.N
    Ca, Cb, ea, eb, dip = (np.ascontiguousarray(x, dtype=np.float64) for x in (*orbitals(g), g["dip"]))
    dim = na * (N - na) + nb * (N - nb)
    e, tdm, osc = np.zeros(dim), np.zeros((dim, 3)), np.zeros(dim)

    def result(with_tdm=False, with_osc=False):
        res = UcisResult()
        res.e = ptr(e)
        if with_tdm:
            res.tdm = ptr(tdm)
        if with_osc:
            res.osc = ptr(osc)
        return res
    res = result()
    good, po, pr = UcisOpts(0, 0), ctypes.byref, ctypes.byref(res)
    C4 = (ptr(Ca), ptr(Cb), ptr(ea), ptr(eb))
    bad = [(po(good), na, nb, -1, 0, *C4, ptr(dip), pr), (po(good), na, nb, 0, nb + 1, *C4, ptr(dip), pr), (po(good), N + 1, nb, 0, 0, *C4, ptr(dip), pr),
           (po(good), na, -1, 0, 0, *C4, ptr(dip), pr), (po(good), 0, 0, 0, 0, *C4, ptr(dip), pr), (po(good), N, N, 0, 0, *C4, ptr(dip), pr),
           (None, na, nb, 0, 0, *C4, ptr(dip), pr), (po(good), na, nb, 0, 0, None, ptr(Cb), ptr(ea), ptr(eb), ptr(dip), pr),
           (po(good), na, nb, 0, 0, ptr(Ca), None, ptr(ea), ptr(eb), ptr(dip), pr), (po(good), na, nb, 0, 0, ptr(Ca), ptr(Cb), None, ptr(eb), ptr(dip), pr),
           (po(good), na, nb, 0, 0, ptr(Ca), ptr(Cb), ptr(ea), None, ptr(dip), pr), (po(good), na, nb, 0, 0, *C4, ptr(dip), None),
           (po(UcisOpts(0, -1)), na, nb, 0, 0, *C4, ptr(dip), pr), (po(good), na, nb, 0, 0, *C4, None, ctypes.byref(result(with_tdm=True))),
           (po(good), na, nb, 0, 0, *C4, None, ctypes.byref(result(with_osc=True)))]
    for args in bad:
        assert L.tf_cis_uhf(ctx, *args) == TF_EINVAL, args
        assert "tf_cis_uhf" in L.tf_last_error(ctx).decode()
        again = engine.cis_uhf(*orbitals(g), na, nb, method="TDHF", dip=g["dip"])                       # the context stays usable
        assert np.array_equal(again["E"], first["E"]) and np.array_equal(again["osc"], first["osc"])
    sres = StabilityResult()
    ps = ctypes.byref(sres)
    bad_u = [(na, nb, -1, 0, *C4, ps), (N + 1, nb, 0, 0, *C4, ps), (0, 0, 0, 0, *C4, ps), (na, nb, 0, 0, None, ptr(Cb), ptr(ea), ptr(eb), ps),
             (na, nb, 0, 0, ptr(Ca), ptr(Cb), ptr(ea), None, ps), (na, nb, 0, 0, *C4, None)]
    for args in bad_u:
        assert L.tf_stability_uhf(ctx, *args) == TF_EINVAL, args
        assert "tf_stability_uhf" in L.tf_last_error(ctx).decode()
        assert engine.stability_uhf(*orbitals(g), na, nb)["lowest"] == first_stab["lowest"]
    bad_r = [(na, -1, ptr(Ca), ptr(ea), ps), (na, na, ptr(Ca), ptr(ea), ps), (0, 0, ptr(Ca), ptr(ea), ps), (N, 0, ptr(Ca), ptr(ea), ps),
             (na, 0, None, ptr(ea), ps), (na, 0, ptr(Ca), None, ps), (na, 0, ptr(Ca), ptr(ea), None)]
    for args in bad_r:
        assert L.tf_stability_rhf(ctx, *args) == TF_EINVAL, args
        assert "tf_stability_rhf" in L.tf_last_error(ctx).decode()
        assert engine.stability_uhf(*orbitals(g), na, nb)["lowest"] == first_stab["lowest"]
    assert L.tf_cis_uhf(None, po(good), na, nb, 0, 0, *C4, ptr(dip), pr) == TF_EINVAL
    assert L.tf_stability_uhf(None, na, nb, 0, 0, *C4, ps) == TF_EINVAL and L.tf_stability_rhf(None, na, 0, ptr(Ca), ptr(ea), ps) == TF_EINVAL
    with Engine(0) as fresh:                                          # no tensor yet
        fresh.set_basis(aos)
        assert fresh._L.tf_cis_uhf(fresh._ctx, po(good), na, nb, 0, 0, *C4, ptr(dip), pr) == TF_EINVAL
        assert fresh._L.tf_stability_uhf(fresh._ctx, na, nb, 0, 0, *C4, ps) == TF_EINVAL
        assert fresh._L.tf_stability_rhf(fresh._ctx, na, 0, ptr(Ca), ptr(ea), ps) == TF_EINVAL
    with Engine(0, 0, 2) as half:                                     # rank 0 of two: sharding is not supported
        half.set_basis(aos).build_eri(True)
        assert half._L.tf_cis_uhf(half._ctx, po(good), na, nb, 0, 0, *C4, ptr(dip), pr) == TF_EINVAL
        assert half._L.tf_stability_uhf(half._ctx, na, nb, 0, 0, *C4, ps) == TF_EINVAL
        assert half._L.tf_stability_rhf(half._ctx, na, 0, ptr(Ca), ptr(ea), ps) == TF_EINVAL
    with pytest.raises(TunaError):
        engine.cis_uhf(*orbitals(g), na, nb, method="CISD")
    # a good call through the bare ABI, with the moments
    full = result(with_tdm=True, with_osc=True)
    assert L.tf_cis_uhf(ctx, po(good), na, nb, 0, 0, *C4, ptr(dip), ctypes.byref(full)) == 0 and full.dim == dim and full.dim_alpha == na * (N - na)
    assert np.array_equal(e, first["E"]) and np.array_equal(osc, first["osc"]) and np.array_equal(tdm, first["tdm"])
    assert engine.eri_storage()["layout"] == "packed"


def stability_block(lines):
    text = "\n".join(lines).split("\n")
    start = next(n for n, s in enumerate(text) if "Stability Analysis" in s) - 1
    end = next(n for n in range(start + 3, len(text)) if text[n].startswith(" ~~~~"))
    return text[start:end + 1]


def test_stab_input_lines(engine, ucis_golden):
    """The STAB keyword on an RHF, a UHF and an MP2 line: the printed block against what the reference prints for the same line (its
    eigenvalues to the five printed places), out.stability against the reference's eigenvalues within the 1e-8 of the input-line tests,
    the block in front of the post-SCF stage, and the refusal on a Kohn-Sham line."""
    from tuna_amd.energy import run
    with open(os.path.join(GOLD, "stability_text.json")) as f:
        texts = {t["line"]: t for t in json.load(f) if t["kind"] == "stability"}
    cases = [("SPE : H H 2.0 : HF STO-3G : STAB", "SPE : H H 2.0 : HF STO-3G : STAB"), ("SPE : C O 1.128 : HF 6-31G : STAB", "SPE : C O 1.128 : HF 6-31G : STAB"),
             ("SPE : O O 1.2075 : UHF STO-3G : ML 3 STAB", "SPE : O O 1.2075 : UHF STO-3G : ML 3 STAB"),
             ("SPE : C O 1.128 : MP2 6-31G : STAB", "SPE : C O 1.128 : HF 6-31G : STAB")]
    for line, key in cases:
        t = texts[key]
        log = []
        out = run(line.replace(": STAB", ": EXTREME STAB").replace("ML 3 STAB", "ML 3 EXTREME COREGUESS STAB"), silent=False, engine=engine, log=log.append)
        st = out.stability
        got = [st["lowest"]] if t["reference"] == "UHF" else [st["lowest_singlet"], st["lowest_triplet"]]
        print(f"\n[{line}] {got} (reference {t['lowest']}) seconds {st['seconds']}")
        assert st["reference"] == t["reference"] and np.abs(np.array(got) - np.array(t["lowest"])).max() < 1e-8
        assert st["stable"] == all(x > -1e-5 for x in t["lowest"]) and st["threshold"] == -1e-5
        same_table(stability_block(log), t["text"].strip("\n").split("\n"))
        text = "\n".join(log)
        if "MP2" in line:
            assert text.index("Stability Analysis") < text.index("MP2 correlation energy") and out.mp2["E_MP2"] < 0
    with pytest.raises(TunaError, match="exchange-correlation kernel"):
        run("SPE : C O 1.128 : B3LYP 6-31G : STAB", engine=engine)


def test_unrestricted_excited_states_through_calculate_energy(engine, ucis_golden):
    """The way in for open shells: calculate_energy with a Calculation whose reference is UHF.  Li/6-31G TDHF and O2/cc-pVDZ CIS with a
    frozen core: out.energy = E_SCF + w_root and every energy against the golden within the 1e-8 Eh of the input-line tests."""
    for tag, symbols, R, basis, ml, method, k, root in (("li_doublet_631g", ["LI"], None, "6-31G", 2, "TDHF", 0, 2),
                                                       ("o2_triplet_ccpvdz", ["O", "O"], SYSTEMS["o2_triplet_ccpvdz"][1], "CC-PVDZ", 3, "CIS", 4, 1)):
        g = ucis_golden[tag]
        calc = energy.interpret_keywords(["EXTREME", "COREGUESS", "ML", str(ml), "ROOT", str(root), "NSTATES", "4"], energy.Calculation("SPE", "HF", basis))
        calc.reference, calc.excited_state, calc.freeze_core = "UHF", method, k > 0
        calc.tamm_dancoff_approximation = method == "CIS"
        log = []
        out = energy.calculate_energy(symbols, R, calc, engine, False, log.append)
        want = g[f"{method}_fc{k}_energies"]
        E_SCF = float(g["E_UHF"])
        print(f"\n[{tag} {method} fc{k}] E = {out.energy:.10f} (golden {E_SCF + want[root - 1]:.10f})")
        assert abs(out.energy - (E_SCF + want[root - 1])) < 1e-8 and np.abs(out.excited["energies"] - want).max() < 1e-8
        assert out.excited["n_frozen"] == k // 2 and out.excited["root"] == root
        X = np.concatenate([out.excited["X_alpha"].ravel(), out.excited["X_beta"].ravel()])
        Y = np.concatenate([out.excited["Y_alpha"].ravel(), out.excited["Y_beta"].ravel()])
        assert abs(np.sum(X * X - Y * Y) - 1) < 1e-12
        text = "\n".join(log)
        assert f"Excitation energy is the energy difference to excited state {root}." in text and text.count("~~~~~ State ") == 4
        assert " - S " not in text and " - T " not in text and re.search(r" \d+[ab]  ->  \d+[ab] ", text)
