"""GPU: closed-shell CIS and TDHF on the resident tensor (tf_cis_rhf: the assembly kernel tfcis::assemble_kernel, the Cholesky
reduction of TDHF on rocSOLVER / rocBLAS, the back-substitution and transition-moment kernels) against the reference program's own
states (tests/golden/cis_systems.npz, cis_text.json) and the independent NumPy checker of tests/cis_reference.py: every energy of
both multiplicities, transition moments by clusters of degenerate states, the assembled matrices and the kept vectors element by
element, n_keep, the multiplicities on their own, the layouts, unstable references, refusals and the input lines of energy.run.  Every
test hands the shared context back with the default layout."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import cis_reference as cr
from conftest import GOLD
from test_cis_reference import CIS_TOL, MOMENT_TOL, R_H2_UNSTABLE, SYSTEMS, TDHF_TOL, UNSTABLE, cluster_sums, frozen_variants, split, system
from test_gpu_mp3 import _random_orbitals, _reset
from tuna_amd import energy
from tuna_amd._lib import CisOpts, CisResult, TunaError, ptr

pytestmark = pytest.mark.gpu

TF_EINVAL, TF_ELINALG = -1, -5
VECTOR_TOL = 1e-8     # elements of X and Y: matrices equal to ~1e-13 per entry give ||dM|| ~ sqrt(dim) 3e-13 < 1e-11; over the smallest gap
#                       of the kept states in w^2 (2 w dw > 0.03) and through L (condition ~ 5) that is below 2e-9


@pytest.fixture(scope="module")
def cis_golden(golden):
    return split(golden("cis_systems"))


@pytest.fixture(scope="module")
def n2_tz():
    shells, aos = system("n2_ccpvtz")
    return aos, cr.dense_eri(aos, shells)


def merged(r):
    return energy.merge_excited_states(r["E_singlet"], r["E_triplet"], r["tdm"], r["osc"])


@pytest.mark.parametrize("tag", list(SYSTEMS))
def test_reference_orbitals_against_goldens(engine, cis_golden, tag):
    """Every energy of both multiplicities (CIS within 1e-10 Eh, TDHF within ten times the deviation of the CPU checker's Cholesky route
    from the golden, 3.6e-12 Eh); |mu| and f as sums over clusters of degenerate states; triplet strengths exactly 0.  N2/STO-3G's
    reference orbitals are an unstable RHF solution (negative CIS energies, which are returned as they are): TDHF refuses it."""
    g = cis_golden[tag]
    engine.set_basis(system(tag)[1]).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed"
    nocc = int(g["n_occ"])
    bad = []
    for nf in frozen_variants(g):
        for method in ("CIS", "TDHF"):
            pre = f"{method}_fc{nf}_"
            if method == "TDHF" and tag in UNSTABLE:
                with pytest.raises(TunaError, match="unstable") as e:
                    engine.cis_rhf(g["C"], g["eps"], nocc, nf, method="TDHF", dip=g["dip"])
                assert e.value.code == TF_ELINALG and "A - B" in str(e.value)
                continue
            r = engine.cis_rhf(g["C"], g["eps"], nocc, nf, method=method, dip=g["dip"])
            tol = CIS_TOL if method == "CIS" else TDHF_TOL
            d = [np.abs(r[f"E_{m}"] - g[pre + f"E_{m}"]).max() for m in ("singlet", "triplet")]
            e, lab, _, mu, f = merged(r)
            ge = g[pre + "energies"]
            d_mu = np.abs(cluster_sums(ge, mu) - cluster_sums(ge, g[pre + "tdm"])).max()
            d_f = np.abs(cluster_sums(ge, f) - cluster_sums(ge, g[pre + "osc"])).max()
            print(f"\n[{tag} {method} fc{nf}] dim {r['dim']} max |dE| singlet {d[0]:.1e} triplet {d[1]:.1e} (tol {tol:.1e}) cluster |mu| d {d_mu:.1e} "
                  f"f d {d_f:.1e} seconds {r['seconds']}")
            assert r["dim"] == len(g[pre + "E_singlet"]) and np.abs(e - ge).max() <= max(d) + 1e-300
            assert np.all(mu[lab == "triplet"] == 0) and np.all(f[lab == "triplet"] == 0)
            assert np.allclose(np.linalg.norm(r["tdm"], axis=1) ** 2 * r["E_singlet"] * (2 / 3), r["osc"], rtol=1e-12, atol=1e-15)
            if not (max(d) < tol and d_mu < MOMENT_TOL and d_f < MOMENT_TOL):
                bad.append((method, nf, d, d_mu, d_f))
    assert not bad, bad


def shifted_random_orbitals(N, width):
    """_random_orbitals with the virtual energies 1 Eh higher: with its own energies the random orbitals of width 8 are triplet
    unstable (min w^2 = -0.001, checked on the CPU) and width 7 is marginal; the wider gap gives min eig(A - B) > 1.2, min w^2 > 1.2 and
    the five lowest states of either multiplicity, CIS and TDHF, more than 1.4e-2 Eh apart in all five cases."""
    C, eps = _random_orbitals(N, 30 + width)
    eps = eps.copy()
    eps[width:] += 1.0
    return C, eps


def up_to_sign(got, want):
    """max |got - s want| with one sign s per state; [n, dim] each"""
    s = np.sign(np.sum(got * want, axis=1))[:, None]
    return np.abs(got - s * want).max()


@pytest.mark.parametrize("width,nf", [(1, 0), (7, 0), (8, 0), (12, 0), (7, 6)])
def test_matrices_and_vectors_against_the_independent_checker(engine, n2_tz, width, nf):
    """N2/cc-pVTZ, random orthonormal orbitals, dim = 59 (one partial tile of 32 x 32), 371 (ragged edges), 416 and 576 (exact multiples
    of the tile), and 53 through the frozen path.  The assembled matrices element by element within 1e-11 max|entry|, bitwise symmetric
    and bit for bit the same in a second call; the five lowest vectors of either multiplicity element by element up to a sign per state,
    X.X - Y.Y = 1 to 1e-12."""
    aos, E = n2_tz
    engine.set_basis(aos).build_eri(True)
    C, eps = shifted_random_orbitals(engine.N, width)
    o, v = width - nf, engine.N - width
    dim, nk = o * v, 5
    m = cr.matrices(E, C, eps, width, nf)
    bad = []
    for method, names in (("CIS", {"M_plus_singlet": "A_singlet", "M_plus_triplet": "A_triplet"}),
                          ("TDHF", {"M_plus_singlet": "plus_singlet", "M_plus_triplet": "plus_triplet", "M_minus": "minus"})):
        r, again = (engine.cis_rhf(C, eps, width, nf, method=method, n_keep=nk, return_matrices=True) for _ in range(2))
        assert r["dim"] == dim and (r["M_minus"] is None) == (method == "CIS")
        for key, kind in names.items():
            M, want = r[key], m[kind]
            scale = np.abs(want).max()
            d = np.abs(M - want).max() / scale
            print(f"\n[o {o} v {v} frozen {nf} {method} {key}] max|entry| {scale:.2f} max|d| / max|entry| {d:.1e}")
            assert np.array_equal(M, M.T), (method, key)
            assert np.array_equal(M, again[key]), (method, key)
            if not d <= 1e-11:
                bad.append((method, key, d))
        for mult in ("singlet", "triplet"):
            assert np.array_equal(r[f"E_{mult}"], again[f"E_{mult}"]) and np.array_equal(r[f"X_{mult}"], again[f"X_{mult}"])
            X, Y = r[f"X_{mult}"].reshape(-1, dim), r[f"Y_{mult}"].reshape(-1, dim)
            k = min(nk, dim)
            assert X.shape == (k, dim)
            if method == "CIS":
                e, V = cr.cis(m[f"A_{mult}"])
                wX, wY, tol = V[:, :k].T, np.zeros((k, dim)), CIS_TOL
            else:
                ref = cr.tdhf_cholesky(m[f"plus_{mult}"], m["minus"])
                assert ref["min_eig_minus"] > 0 and ref["min_w2"] > 0
                e, wX, wY, tol = ref["E"], ref["X"][:, :k].T, ref["Y"][:, :k].T, 1e-10
            assert k < 2 or np.diff(e[:k + 1]).min() > 1e-6
            dE = np.abs(r[f"E_{mult}"] - e).max()
            dX = up_to_sign(X, wX)
            s = np.sign(np.sum(X * wX, axis=1))[:, None]
            dY = np.abs(Y - s * wY).max()
            norm = np.abs(np.sum(X * X - Y * Y, axis=1) - 1).max()
            print(f"[o {o} v {v} frozen {nf} {method} {mult}] max |dE| {dE:.1e} max |dX| {dX:.1e} max |dY| {dY:.1e} |X.X - Y.Y - 1| {norm:.1e}")
            if method == "CIS":
                assert not Y.any()
            if not (dE < tol and dX < VECTOR_TOL and dY < VECTOR_TOL and norm < 1e-12):
                bad.append((method, mult, dE, dX, dY, norm))
    assert not bad, bad


def test_n_keep_and_single_multiplicities(engine, cis_golden):
    """n_keep = 0, 1 and dim (and beyond: clamped); singlets only and triplets only give the energies of the combined call bit for bit."""
    g = cis_golden["co_631g"]
    engine.set_basis(system("co_631g")[1]).build_eri(True)
    nocc, dim = 7, 77
    for method in ("CIS", "TDHF"):
        both = engine.cis_rhf(g["C"], g["eps"], nocc, 0, method=method, n_keep=dim, dip=g["dip"])
        assert both["X_singlet"].shape == both["Y_triplet"].shape == (dim, 7, 11)
        for mult in ("singlet", "triplet"):
            X, Y = both[f"X_{mult}"].reshape(dim, dim), both[f"Y_{mult}"].reshape(dim, dim)
            assert np.abs(np.sum(X * X - Y * Y, axis=1) - 1).max() < 1e-12
            if method == "CIS":
                assert np.abs(X @ X.T - np.eye(dim)).max() < 1e-12 and not Y.any()
            else:
                assert np.abs(X @ X.T - Y @ Y.T - np.eye(dim)).max() < 1e-10      # the states are (X, Y)-orthonormal in the TDHF metric
        none = engine.cis_rhf(g["C"], g["eps"], nocc, 0, method=method, n_keep=0, dip=g["dip"])
        one = engine.cis_rhf(g["C"], g["eps"], nocc, 0, method=method, n_keep=1)
        many = engine.cis_rhf(g["C"], g["eps"], nocc, 0, method=method, n_keep=dim + 5)
        assert none["X_singlet"] is None and none["Y_triplet"] is None and one["tdm"] is None and one["osc"] is None
        # (the triangular solve behind X - Y takes another route for one right-hand side than for many: the same vectors, not the same bits)
        assert one["X_singlet"].shape == (1, 7, 11) and np.abs(one["X_triplet"][0] - both["X_triplet"][0]).max() < 1e-12
        assert np.abs(one["Y_singlet"][0] - both["Y_singlet"][0]).max() < 1e-12 and np.array_equal(many["X_singlet"], both["X_singlet"])
        s_only = engine.cis_rhf(g["C"], g["eps"], nocc, 0, method=method, triplets=False, n_keep=2, dip=g["dip"])
        t_only = engine.cis_rhf(g["C"], g["eps"], nocc, 0, method=method, singlets=False, n_keep=2, dip=g["dip"])
        for r in (none, one, many, s_only):
            assert np.array_equal(r["E_singlet"], both["E_singlet"])
        for r in (none, one, many, t_only):
            assert np.array_equal(r["E_triplet"], both["E_triplet"])
        assert s_only["E_triplet"] is None and s_only["X_triplet"] is None and t_only["E_singlet"] is None and t_only["tdm"] is None
        assert np.array_equal(s_only["osc"], both["osc"]) and np.array_equal(s_only["tdm"], both["tdm"]) and np.array_equal(none["osc"], both["osc"])
        assert np.abs(s_only["X_singlet"] - both["X_singlet"][:2]).max() < 1e-12 and np.abs(t_only["Y_triplet"] - both["Y_triplet"][:2]).max() < 1e-12


def test_layouts_agree(engine, cis_golden):
    g = cis_golden["n2_ccpvdz"]
    aos = system("n2_ccpvdz")[1]
    try:
        e = {}
        for layout in ("packed", "rows", "tiles"):
            engine.set_basis(aos).build_eri(True, layout=layout)
            assert engine.eri_storage()["layout"] == layout
            e[layout] = {method: engine.cis_rhf(g["C"], g["eps"], 7, 1, method=method, dip=g["dip"]) for method in ("CIS", "TDHF")}
        for method, tol in (("CIS", CIS_TOL), ("TDHF", TDHF_TOL)):
            for lt in ("packed", "rows", "tiles"):
                d = max(np.abs(e[lt][method][f"E_{m}"] - g[f"{method}_fc1_E_{m}"]).max() for m in ("singlet", "triplet"))
                print(f"\n[{method}] {lt} against the golden {d:.1e}")
                assert d < tol
                assert abs(e[lt][method]["osc"].sum() - g[f"{method}_fc1_osc"].sum()) < MOMENT_TOL
    finally:
        _reset(engine)
    engine.set_basis(aos).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed"


def test_unstable_reference(engine):
    """H2/STO-3G at 2.0 angstrom, past the Coulson-Fischer point (1.2 angstrom in this basis; found with the CPU checker): A - B = 0.1184
    > 0, triplet w^2 = -0.0473 < 0, singlet w^2 = 0.0754.  TDHF raises TF_ELINALG and says unstable, CIS on the same orbitals returns
    the checker's negative lowest triplet energy (-0.1407 Eh), TDHF of the singlets alone runs, and the context is unaffected."""
    aos, E, C, eps = cr.h2_minimal_basis(R_H2_UNSTABLE)
    m = cr.matrices(E, C, eps, 1, 0)
    rt, rs = cr.tdhf_cholesky(m["plus_triplet"], m["minus"]), cr.tdhf_cholesky(m["plus_singlet"], m["minus"])
    assert rt["min_eig_minus"] > 0 and rt["min_w2"] < 0 < rs["min_w2"] and m["A_triplet"][0, 0] < 0
    engine.set_basis(aos).build_eri(True)
    first = engine.cis_rhf(C, eps, 1, 0, method="CIS")
    assert first["E_triplet"][0] < 0 and abs(first["E_triplet"][0] - m["A_triplet"][0, 0]) < CIS_TOL
    assert abs(first["E_singlet"][0] - m["A_singlet"][0, 0]) < CIS_TOL
    for kw in ({}, dict(singlets=False)):
        with pytest.raises(TunaError, match="unstable") as e:
            engine.cis_rhf(C, eps, 1, 0, method="TDHF", **kw)
        print("\n" + str(e.value))
        assert e.value.code == TF_ELINALG and "triplet" in str(e.value) and "w^2" in str(e.value)
        assert f"{rt['min_w2']:.6f}"[:8] in str(e.value)
    s_only = engine.cis_rhf(C, eps, 1, 0, method="TDHF", triplets=False, n_keep=1)
    assert abs(s_only["E_singlet"][0] - rs["E"][0]) < TDHF_TOL
    again = engine.cis_rhf(C, eps, 1, 0, method="CIS")
    assert again["E_triplet"][0] == first["E_triplet"][0] and again["E_singlet"][0] == first["E_singlet"][0]


def test_refusals(engine, cis_golden):
    from tuna_amd.engine import Engine
    g = cis_golden["hf_ccpvdz"]
    aos = system("hf_ccpvdz")[1]
    engine.set_basis(aos).build_eri(True)
    nocc = 5
    first = engine.cis_rhf(g["C"], g["eps"], nocc, 0, method="TDHF", dip=g["dip"])
    L, ctx, N = engine._L, engine._ctx, engine.N
    C, eps, dip = (np.ascontiguousarray(x, dtype=np.float64) for x in (g["C"], g["eps"], g["dip"]))
    dim = nocc * (N - nocc)
    e_s, e_t, tdm, osc = np.zeros(dim), np.zeros(dim), np.zeros((dim, 3)), np.zeros(dim)

    def result(with_moments=False):
        res = CisResult()
        res.e_singlet, res.e_triplet = ptr(e_s), ptr(e_t)
        if with_moments:
            res.tdm, res.osc = ptr(tdm), ptr(osc)
        return res

    def opts(tda=0, singlets=1, triplets=1, n_keep=0):
        return CisOpts(tda, singlets, triplets, n_keep)
    res, with_tdm, with_osc = result(), result(), result()
    with_tdm.tdm, with_osc.osc = ptr(tdm), ptr(osc)
    good, po, pr = opts(), ctypes.byref, ctypes.byref(res)
    bad = [(po(good), nocc, -1, ptr(C), ptr(eps), ptr(dip), pr), (po(good), nocc, nocc, ptr(C), ptr(eps), ptr(dip), pr),
           (po(good), 0, 0, ptr(C), ptr(eps), ptr(dip), pr), (po(good), N, 0, ptr(C), ptr(eps), ptr(dip), pr),
           (None, nocc, 0, ptr(C), ptr(eps), ptr(dip), pr), (po(good), nocc, 0, None, ptr(eps), ptr(dip), pr),
           (po(good), nocc, 0, ptr(C), None, ptr(dip), pr), (po(good), nocc, 0, ptr(C), ptr(eps), ptr(dip), None),
           (po(opts(singlets=0, triplets=0)), nocc, 0, ptr(C), ptr(eps), ptr(dip), pr), (po(opts(n_keep=-1)), nocc, 0, ptr(C), ptr(eps), ptr(dip), pr),
           (po(good), nocc, 0, ptr(C), ptr(eps), None, ctypes.byref(with_tdm)), (po(good), nocc, 0, ptr(C), ptr(eps), None, ctypes.byref(with_osc))]
    for args in bad:
        assert L.tf_cis_rhf(ctx, *args) == TF_EINVAL, args
        assert "tf_cis_rhf" in L.tf_last_error(ctx).decode()
        again = engine.cis_rhf(g["C"], g["eps"], nocc, 0, method="TDHF", dip=g["dip"])       # the context stays usable
        assert np.array_equal(again["E_singlet"], first["E_singlet"]) and np.array_equal(again["E_triplet"], first["E_triplet"])
        assert np.array_equal(again["osc"], first["osc"])
    assert L.tf_cis_rhf(None, po(good), nocc, 0, ptr(C), ptr(eps), ptr(dip), pr) == TF_EINVAL
    with Engine(0) as fresh:                                          # no tensor yet
        fresh.set_basis(aos)
        assert fresh._L.tf_cis_rhf(fresh._ctx, po(good), nocc, 0, ptr(C), ptr(eps), ptr(dip), pr) == TF_EINVAL
    with Engine(0, 0, 2) as half:                                     # rank 0 of two: sharding is not supported
        half.set_basis(aos).build_eri(True)
        assert half._L.tf_cis_rhf(half._ctx, po(good), nocc, 0, ptr(C), ptr(eps), ptr(dip), pr) == TF_EINVAL
    with pytest.raises(TunaError):
        engine.cis_rhf(g["C"], g["eps"], nocc, 0, method="CISD")
    with pytest.raises(TunaError) as e:
        engine.cis_rhf(g["C"], g["eps"], nocc, 0, singlets=False, triplets=False)
    assert e.value.code == TF_EINVAL and "no excited states" in str(e.value)
    # a good call through the bare ABI, with the moments
    full = result(with_moments=True)
    assert L.tf_cis_rhf(ctx, po(good), nocc, 0, ptr(C), ptr(eps), ptr(dip), ctypes.byref(full)) == 0 and full.dim == dim
    assert np.array_equal(e_s, first["E_singlet"]) and np.array_equal(e_t, first["E_triplet"]) and np.array_equal(osc, first["osc"])
    assert engine.eri_storage()["layout"] == "packed"


NUMBER = re.compile(r"-?\d+\.\d+")


def same_table(got, want):
    """The spectrum rows agree: the same layout, and every number within one unit of its last printed place plus 1e-7 of its value (the
    orbitals of a line's own SCF fix the excitation energies to the 1e-8 Eh of the input-line tests)."""
    assert len(got) == len(want), (got, want)
    for a, b in zip(got, want):
        assert NUMBER.sub("#", a).split() == NUMBER.sub("#", b).split() and len(a) == len(b), (a, b)
        for x, y in zip(NUMBER.findall(a), NUMBER.findall(b)):
            places = len(y.split(".")[1])
            assert abs(float(x) - float(y)) <= 1.01 * 10.0 ** -places + 1e-7 * abs(float(y)), (a, b)


def spectrum_rows(lines):
    text = "\n".join(lines).split("\n")
    start = next(n for n, s in enumerate(text) if s.startswith("   State         Energy"))
    rows = []
    for s in text[start + 2:]:
        if s.startswith(" ~~~~"):
            break
        rows.append(s)
    return rows


def test_input_lines(engine, cis_golden):
    """out.energy = E_SCF + w_root against the golden within the 1e-8 Eh of the project's input-line tests; the printed spectrum against
    what the reference prints; contribution lines for the states that are not degenerate in the golden, summed over blocks of
    degenerate orbitals (48.39 + 48.39 % here against 24.87 + 23.53 + 23.53 + 24.87 % there is the same pi -> pi* state in rotated pi
    orbitals)."""
    from tuna_amd.energy import run
    with open(os.path.join(GOLD, "cis_text.json")) as f:
        texts = {t["line"]: t for t in json.load(f)}
    g = cis_golden["co_631g"]
    E_SCF = float(g["E_SCF"])
    cases = [("SPE : C O 1.128 : CIS 6-31G : EXTREME", "CIS_fc0_", 1, None, "SPE : C O 1.128 : CIS 6-31G"),
             ("SPE : C O 1.128 : TDHF 6-31G : EXTREME NSTATES 5 ROOT 2", "TDHF_fc0_", 2, None, "SPE : C O 1.128 : TDHF 6-31G : NSTATES 5"),
             ("SPE : C O 1.128 : HF 6-31G : EXTREME TD TDA NOTRIPLETS", "CIS_fc0_", 1, 0, None)]
    for line, pre, root, only, text_key in cases:
        log = []
        out = run(line, silent=False, engine=engine, log=log.append)
        ge, lab = g[pre + "energies"], g[pre + "labels"]
        keep = lab == only if only is not None else np.ones(len(ge), bool)
        want = ge[keep]
        print(f"\n[{line}] E = {out.energy:.10f} (golden {E_SCF + want[root - 1]:.10f}, d {out.energy - E_SCF - want[root - 1]:.1e}) seconds "
              f"{out.excited['seconds']}")
        assert abs(out.energy - (E_SCF + want[root - 1])) < 1e-8, (line, out.energy, E_SCF + want[root - 1])
        assert np.abs(out.excited["energies"] - want).max() < 1e-8 and out.excited["root"] == root
        d_f = np.abs(cluster_sums(want, out.excited["oscillator_strengths"]) - cluster_sums(want, g[pre + "osc"][keep])).max()
        assert d_f < MOMENT_TOL
        X, Y = out.excited["X"], out.excited["Y"]
        assert abs(np.sum(X * X - Y * Y) - 1) < 1e-12
        text = "\n".join(log)
        assert f"Excitation energy is the energy difference to excited state {root}." in text and "Final single point energy:" in text
        name = {"CIS": "CIS:", "TDHF": "TDHF:", "HF": "TD-HF:"}[line.split(":")[2].split()[0]]
        assert f" Excitation energy from {name:<11} {out.excited['E_transition']:15.10f}" in text
        if only == 0:
            assert "Only singlet states will be calculated." in text and "Using the Tamm-Dancoff approximation..." in text
            assert " - T " not in text and text.count("~~~~~ State ") == 10
        if text_key:
            ref = texts[text_key]["text"].split("\n")
            # a singlet and a triplet can be exactly degenerate (the Sigma- states of CO): inside a cluster of the golden the rows are
            # compared without their state numbers, in the order of their labels
            rows, ref_rows = spectrum_rows(log), spectrum_rows(ref)
            assert [r[:5] for r in rows] == [r[:5] for r in ref_rows]
            for c in cr.clusters(want[:len(ref_rows)]):
                same_table(sorted(rows[n][5:] for n in c), sorted(ref_rows[n][5:] for n in c))
            # the contribution blocks of the states that stand alone in the golden
            mine, theirs = text.split("\n"), ref
            n_states = texts[text_key]["n_states"]
            alone = [c[0] for c in cr.clusters(ge) if len(c) == 1 and c[0] < n_states]
            assert alone

            def block(lines, n):
                start = next(k for k, s in enumerate(lines) if s.startswith(f"  ~~~~~ State {n + 1} ~~~~~"))
                rows = {}
                for s in lines[start + 4:]:
                    if "->" not in s:
                        break
                    i, _, a, value, _ = s.split()
                    rows[(i, a)] = float(value)
                return lines[start], rows
            # A state that stands alone is still written in orbitals that do not: the pi and pi* pairs of CO are defined up to a
            # rotation, and a line's own SCF need not return the golden's.  What the rotation leaves alone is the sum over a block of
            # degenerate occupied x degenerate virtual orbitals, so the rows are compared block by block: within one unit of the last
            # printed place per row, plus EXTHRESH (1 %) for every pair of the block that one side did not print.
            group = {}
            for c in cr.clusters(g["eps"]):
                for k in c:
                    group[str(k + 1)] = (c[0], len(c))
            for n in alone:
                (head, rows), (ref_head, ref_rows) = block(mine, n), block(theirs, n)
                assert head == ref_head, (n, head, ref_head)
                sums = {}
                for side, table in enumerate((rows, ref_rows)):
                    for (i, a), value in table.items():
                        entry = sums.setdefault((group[i], group[a]), [0.0, 0.0, 0, 0])
                        entry[side] += value
                        entry[2 + side] += 1
                for ((_, ni), (_, na)), (mine_sum, ref_sum, n_mine, n_ref) in sums.items():
                    tol = 0.0101 * max(n_mine, n_ref) + 1.0 * (ni * na - min(n_mine, n_ref))
                    assert abs(mine_sum - ref_sum) <= tol, (n, rows, ref_rows)
                    if ni * na == 1 and n_mine == n_ref == 1:
                        assert abs(mine_sum - ref_sum) <= 0.0101, (n, rows, ref_rows)
    for line in ("SPE : C O 1.128 : CIS(D) 6-31G", "SPE : C O 1.128 : UCIS 6-31G", "SPE : O O 1.2075 : TDHF STO-3G : ML 3",
                 "SPE : C O 1.128 : B3LYP 6-31G : TD", "SPE : C O 1.128 : CIS 6-31G : DIPOLE", "SPE : C O 1.128 : CIS 6-31G : NOSINGLETS NOTRIPLETS",
                 "SPE : C O 1.128 : CIS 6-31G : ROOT 155", "SPE : C O 1.128 : CISD 6-31G"):
        with pytest.raises(TunaError):
            run(line, engine=engine)
    with pytest.raises(TunaError, match=r"Specified root \(155\) does not exist!"):
        run("SPE : C O 1.128 : CIS 6-31G : ROOT 155", engine=engine)
