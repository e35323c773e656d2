"""GPU: restricted LCCD and CCD iterated on the resident tensor (tf_ccd_rhf) against the reference program's own iteration
(tests/golden/ccd_systems.npz) and the independent NumPy iteration of tests/ccd_reference.py: converged energies, the energy of every
step and the step count; LCCD's first step against tf_mp3_rhf; the amplitudes of fixed numbers of steps element by element; the layouts
against each other; DIIS, NODIIS and damping; repeatability; refusals; the input lines of energy.run.  Every test hands the shared context
back with the default layout."""
import ctypes

import numpy as np
import pytest

import ccd_reference as cr
import mp3_reference as mr
from test_ccd_reference import split
from test_gpu_mp3 import SYSTEMS, _random_orbitals, _reset, _system
from tuna_amd._lib import CcOpts, CcResult, TunaError, ptr

pytestmark = pytest.mark.gpu

TF_EINVAL, TF_ENOTCONV = -1, -4
METHODS = ("LCCD", "CCD")
GOLD = dict(conv_delta_E=1e-11, conv_amplitudes=1e-10, use_diis=True, max_diis=6)     # the thresholds of tools/make_golden_ccd.py


@pytest.fixture(scope="module")
def ccd_golden(golden):
    return split(golden("ccd_systems"))


@pytest.fixture(scope="module")
def mp3_golden(golden):
    return split(golden("mp3_systems"))


@pytest.fixture(scope="module")
def n2_tz():
    shells, aos = _system("n2_ccpvtz")
    return aos, mr.dense_eri(aos, shells)


def check_against_golden(r, g, pre, what, conv_delta_E=1e-11, conv_amplitudes=1e-10):
    """|E_corr - golden| < 1e-9; every step within 1e-8; step counts equal, or one apart where the golden's deciding quantity -- the larger
    of |dE| and ||dt|| over their thresholds -- sits within a factor 2 of its threshold at the step where one side stopped"""
    want, dts = g[pre + "energies"], g[pre + "dt_norms"]
    n, ng = r["n_iter"], int(g[pre + "n_iter"])
    m = min(n, ng)
    step_diff = np.abs(r["table"][:m, 1] - want[:m]).max()
    print(f"\n[{what}] E_corr {r['E_corr']:.12f} golden {float(g[pre + 'E_corr']):.12f} d {r['E_corr'] - float(g[pre + 'E_corr']):.1e} steps {n} "
          f"golden {ng} max step d {step_diff:.1e}")
    assert r["converged"], what
    assert abs(r["E_corr"] - float(g[pre + "E_corr"])) < 1e-9, what
    assert step_diff < 1e-8, what
    assert np.array_equal(r["table"][:, 0], np.arange(1, n + 1)) and np.allclose(np.diff(np.concatenate([[0.0], r["table"][:, 1]])), r["table"][:, 2],
                                                                               rtol=0, atol=1e-15)
    if n != ng:
        assert abs(n - ng) == 1, what
        k = min(n, ng) - 1                                                # the step at which one side stopped and the other went on
        dE = abs(want[k] - (want[k - 1] if k else 0.0))
        ratios = (dE / conv_delta_E, dts[k] / conv_amplitudes)
        print(f"[{what}] step counts differ: golden |dE| / threshold {ratios[0]:.2f}, ||dt|| / threshold {ratios[1]:.2f} at step {k + 1}")
        assert 0.5 < max(ratios) < 2.0, (what, ratios)


@pytest.mark.parametrize("tag", ["n2_ccpvdz", "n2_ccpvtz", "co_631g", "hf_ccpvdz", "ne_ccpvdz"])
def test_reference_orbitals_against_goldens(engine, ccd_golden, mp3_golden, tag):
    g, m = ccd_golden[tag], mp3_golden[tag]
    engine.set_basis(_system(tag)[1]).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed"
    nocc = int(m["n_occ"])
    for method in METHODS:
        for nf in (0, 1):
            r = engine.ccd_rhf(m["C"], m["eps"], nocc, nf, method=method, **GOLD)
            check_against_golden(r, g, f"{method}_fc{nf}_", f"{tag} {method} fc{nf}")
            m2 = engine.mp2_rhf(m["C"], m["eps"], nocc, nf)
            rel = abs(r["E_MP2"] - m2["E_MP2"]) / abs(m2["E_MP2"])
            print(f"[{tag} {method} fc{nf}] E_MP2 {r['E_MP2']:.12f} mp2_rhf {m2['E_MP2']:.12f} rel {rel:.1e} seconds {r['seconds']}")
            assert rel < 1e-12


def test_golden_file_holds_the_required_systems(ccd_golden):
    assert {"n2_ccpvdz", "n2_ccpvtz", "hf_ccpvdz", "ne_ccpvdz"} <= set(ccd_golden) <= set(SYSTEMS)


def test_lccd_step_one_is_mp2_plus_mp3(engine, mp3_golden, n2_tz):
    m = mp3_golden["n2_ccpvtz"]
    engine.set_basis(n2_tz[0]).build_eri(True)
    for nf in (0, 1):
        r = engine.ccd_rhf(m["C"], m["eps"], 7, nf, method="LCCD", max_iter=1, allow_unconverged=True)
        r3 = engine.mp3_rhf(m["C"], m["eps"], 7, nf)
        want = r3["E_OS"] + r3["E_SS"] + r3["E_MP3"]
        rel = abs(r["table"][0, 1] - want) / abs(want)
        print(f"\n[N2/cc-pVTZ fc{nf}] LCCD step 1 {r['table'][0, 1]:.13f} MP2 + MP3 {want:.13f} rel {rel:.1e}")
        assert r["n_iter"] == 1 and not r["converged"] and r["table"].shape == (1, 3) and r["E_corr"] == r["table"][0, 1]
        assert rel < 1e-11


LOOPS = {"two plain steps": (2, dict(use_diis=False), {}),
         "three steps, DIIS and damping 0.2": (3, dict(use_diis=True, damping=0.2), dict(diis=True, damping=0.2)),
         # the last amplitudes of a run are never extrapolated, so three steps reach the damping alone: six steps go through three
         # extrapolations (the history growing from three vectors to five)
         "six steps, DIIS and damping 0.2": (6, dict(use_diis=True, damping=0.2), dict(diis=True, damping=0.2))}


@pytest.mark.parametrize("width", [1, 7, 8, 12])
def test_fixed_steps_against_the_independent_checker(engine, n2_tz, width):
    """N2/cc-pVTZ, random orthonormal orbitals (max |t| stays below 0.15 over these steps, checked on the CPU): one pair; 49 pairs (one
    partial batch of the ladder); 64 pairs (one full batch); 144 pairs (three batches, the last one partial)."""
    aos, E = n2_tz
    engine.set_basis(aos).build_eri(True)
    C, eps = _random_orbitals(engine.N, 30 + width)
    bad = []
    for method in METHODS:
        for what, (k, gpu_loop, ref_loop) in LOOPS.items():
            r = engine.ccd_rhf(C, eps, width, 0, method=method, max_iter=k, conv_delta_E=0.0, conv_amplitudes=0.0, return_t2=True,
                               allow_unconverged=True, **gpu_loop)
            ref = cr.restricted_iterations(E, C, eps, width, 0, method, k, **ref_loop)
            scale = np.abs(ref["t"]).max()
            dt = np.abs(r["t2"] - ref["t"]).max() / scale
            dE = np.abs(r["table"][:, 1] - np.array(ref["energies"])) / np.abs(ref["energies"])
            print(f"\n[width {width} {method}, {what}] max|t| {scale:.3f} max|dt|/max|t| {dt:.1e} rel dE per step {dE}")
            assert scale < 1.0 and r["n_iter"] == k and not r["converged"]
            if not (dt <= 1e-10 and np.all(dE <= 1e-11)):
                bad.append((method, what, dt, dE))
            assert np.array_equal(r["t2"], r["t2"].transpose(1, 0, 3, 2))
    assert not bad, bad


def test_small_diis_depths(engine, mp3_golden):
    """N2/cc-pVDZ (N = 28, o = 7, v = 21), golden orbitals, packed layout: ten fixed steps with damping 0.2 at max_diis 1, 2 and 3, where
    the history drops a vector in every step from the third on (the fixed-step loops above never drop one, the golden runs keep six).
    Against the checker's own loop at the same depth, element by element, with the tolerances of the test above; and the runs at depth 1
    and 2 are the same loop (two vectors kept, one leaving per step), so they agree bit for bit.  The checker's two forms
    (restricted_iterations, iterations_from_blocks) agree to 4e-15 in t and 4e-16 in E over these ten steps, max|t| = 0.076."""
    m = mp3_golden["n2_ccpvdz"]
    shells, aos = _system("n2_ccpvdz")
    E = mr.dense_eri(aos, shells)
    engine.set_basis(aos).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed"
    bad = []
    for method in METHODS:
        runs = {}
        for depth in (1, 2, 3):
            r = engine.ccd_rhf(m["C"], m["eps"], 7, 0, method=method, max_iter=10, conv_delta_E=0.0, conv_amplitudes=0.0, return_t2=True,
                               allow_unconverged=True, use_diis=True, max_diis=depth, damping=0.2)
            ref = cr.restricted_iterations(E, m["C"], m["eps"], 7, 0, method, 10, diis=True, max_diis=depth, damping=0.2)
            scale = np.abs(ref["t"]).max()
            dt = np.abs(r["t2"] - ref["t"]).max() / scale
            dE = np.abs(r["table"][:, 1] - np.array(ref["energies"])) / np.abs(ref["energies"])
            print(f"\n[{method}, max_diis {depth}] max|t| {scale:.3f} max|dt|/max|t| {dt:.1e} rel dE per step {dE}")
            assert scale < 1.0 and r["n_iter"] == 10 and not r["converged"]
            if not (dt <= 1e-10 and np.all(dE <= 1e-11)):
                bad.append((method, depth, dt, dE))
            runs[depth] = r
        assert np.array_equal(runs[1]["t2"], runs[2]["t2"]) and np.array_equal(runs[1]["table"], runs[2]["table"]), method
        assert not np.array_equal(runs[2]["t2"], runs[3]["t2"]), method      # (the depth does reach the loop)
    assert not bad, bad


def test_layouts_agree(engine, mp3_golden, n2_tz):
    m = mp3_golden["n2_ccpvtz"]
    try:
        e = {}
        for layout in ("packed", "rows", "tiles"):
            engine.set_basis(n2_tz[0]).build_eri(True, layout=layout)
            assert engine.eri_storage()["layout"] == layout
            e[layout] = {method: engine.ccd_rhf(m["C"], m["eps"], 7, 1, method=method, **GOLD) for method in METHODS}
        for method in METHODS:
            for lt in ("rows", "tiles"):
                d = abs(e[lt][method]["E_corr"] - e["packed"][method]["E_corr"])
                print(f"\n[{method}] {lt} - packed {d:.1e} steps {e[lt][method]['n_iter']} / {e['packed'][method]['n_iter']}")
                assert d < 1e-10 and e[lt][method]["converged"]
    finally:
        _reset(engine)
    engine.set_basis(n2_tz[0]).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed"


def test_diis_nodiis_and_damping(engine, ccd_golden, mp3_golden):
    g, m = ccd_golden["n2_ccpvdz"], mp3_golden["n2_ccpvdz"]
    engine.set_basis(_system("n2_ccpvdz")[1]).build_eri(True)
    for method in METHODS:
        with_diis = engine.ccd_rhf(m["C"], m["eps"], 7, 0, method=method, **GOLD)
        plain = engine.ccd_rhf(m["C"], m["eps"], 7, 0, method=method, **dict(GOLD, use_diis=False))
        damped = engine.ccd_rhf(m["C"], m["eps"], 7, 0, method=method, damping=0.3, **GOLD)
        check_against_golden(with_diis, g, f"{method}_fc0_", f"{method} DIIS")
        check_against_golden(plain, g, f"{method}_nodiis_", f"{method} NODIIS")
        check_against_golden(damped, g, f"{method}_damp03_", f"{method} CORRDAMP 0.3")
        assert plain["n_iter"] >= with_diis["n_iter"]


def test_repeatable(engine, mp3_golden):
    m = mp3_golden["n2_ccpvdz"]
    engine.set_basis(_system("n2_ccpvdz")[1]).build_eri(True)
    for method in METHODS:
        a, b = (engine.ccd_rhf(m["C"], m["eps"], 7, 0, method=method, return_t2=True, damping=0.1, **GOLD) for _ in range(2))
        assert a["n_iter"] == b["n_iter"] and np.array_equal(a["table"], b["table"]) and np.array_equal(a["t2"], b["t2"])
        assert a["E_corr"] == b["E_corr"] and a["E_MP2"] == b["E_MP2"]


def test_refusals(engine, ccd_golden, mp3_golden):
    from tuna_amd.engine import Engine
    g, m = ccd_golden["n2_ccpvdz"], mp3_golden["n2_ccpvdz"]
    shells, aos = _system("n2_ccpvdz")
    engine.set_basis(aos).build_eri(True)
    first = engine.ccd_rhf(m["C"], m["eps"], 7, 0, method="CCD", **GOLD)
    L, ctx, N = engine._L, engine._ctx, engine.N
    C, eps = (np.ascontiguousarray(x, dtype=np.float64) for x in (m["C"], m["eps"]))

    def opts(method=1, max_iter=100):
        return CcOpts(method, max_iter, 1, 6, 1e-11, 1e-10, 0.0)
    res = CcResult()
    good, po, pr = opts(), ctypes.byref, ctypes.byref(res)
    bad = [(po(good), 7, -1, ptr(C), ptr(eps), pr), (po(good), 7, 7, ptr(C), ptr(eps), pr), (po(good), 0, 0, ptr(C), ptr(eps), pr),
           (po(good), N, 0, ptr(C), ptr(eps), pr), (None, 7, 0, ptr(C), ptr(eps), pr), (po(good), 7, 0, None, ptr(eps), pr),
           (po(good), 7, 0, ptr(C), None, pr), (po(good), 7, 0, ptr(C), ptr(eps), None), (po(opts(max_iter=0)), 7, 0, ptr(C), ptr(eps), pr),
           (po(opts(method=2)), 7, 0, ptr(C), ptr(eps), pr), (po(opts(method=-1)), 7, 0, ptr(C), ptr(eps), pr)]
    for args in bad:
        assert L.tf_ccd_rhf(ctx, *args) == TF_EINVAL, args
        again = engine.ccd_rhf(m["C"], m["eps"], 7, 0, method="CCD", **GOLD)          # the context stays usable
        assert again["E_corr"] == first["E_corr"] and again["n_iter"] == first["n_iter"]
    assert L.tf_ccd_rhf(None, po(good), 7, 0, ptr(C), ptr(eps), pr) == TF_EINVAL
    with Engine(0) as fresh:                                          # no tensor yet
        fresh.set_basis(aos)
        assert fresh._L.tf_ccd_rhf(fresh._ctx, po(good), 7, 0, ptr(C), ptr(eps), pr) == TF_EINVAL
    with Engine(0, 0, 2) as half:                                     # rank 0 of two: sharding is not supported
        half.set_basis(aos).build_eri(True)
        assert half._L.tf_ccd_rhf(half._ctx, po(good), 7, 0, ptr(C), ptr(eps), pr) == TF_EINVAL
    with pytest.raises(TunaError):
        engine.ccd_rhf(m["C"], m["eps"], 7, 0, method="CCSD")
    # two steps at tight thresholds: not converged, the outputs hold the second step
    table = np.zeros((2, 3))
    res2 = CcResult()
    res2.table = ptr(table)
    assert L.tf_ccd_rhf(ctx, po(opts(max_iter=2)), 7, 0, ptr(C), ptr(eps), ctypes.byref(res2)) == TF_ENOTCONV
    assert res2.n_iter == 2 and not res2.converged and res2.e_corr == table[1, 1] and np.all(table[:, 0] == [1, 2])
    assert np.abs(table[:, 1] - g["CCD_fc0_energies"][:2]).max() < 1e-8
    with pytest.raises(TunaError) as e:
        engine.ccd_rhf(m["C"], m["eps"], 7, 0, method="CCD", max_iter=2, **GOLD)
    assert e.value.code == TF_ENOTCONV
    r = engine.ccd_rhf(m["C"], m["eps"], 7, 0, method="CCD", max_iter=2, allow_unconverged=True, **GOLD)
    assert r["n_iter"] == 2 and not r["converged"] and np.array_equal(r["table"], table)
    again = engine.ccd_rhf(m["C"], m["eps"], 7, 0, method="CCD", **GOLD)
    assert again["E_corr"] == first["E_corr"] and abs(again["E_corr"] - float(g["CCD_fc0_E_corr"])) < 1e-9
    assert engine.eri_storage()["layout"] == "packed"


def test_input_lines(engine, ccd_golden, mp3_golden):
    from tuna_amd.energy import run
    g, E_SCF = ccd_golden["n2_ccpvdz"], float(mp3_golden["n2_ccpvdz"]["E_SCF"])
    cases = [("SPE : N N 1.0977 : CCD CC-PVDZ : TIGHT", "CCD_fc0_"), ("SPE : N N 1.0977 : LCCD CC-PVDZ : TIGHT AMPCONV 1e-10", "LCCD_fc0_"),
             ("SPE : N N 1.0977 : CCD CC-PVDZ : TIGHT NODIIS CORRMAXITER 200", "CCD_nodiis_"),
             ("SPE : N N 1.0977 : CCD CC-PVDZ : TIGHT CORRDAMP 0.3", "CCD_damp03_")]
    text = []
    for line, pre in cases:
        log = []
        out = run(line, silent=False, engine=engine, log=log.append)
        want = E_SCF + float(g[pre + "E_corr"])
        print(f"\n[{line}] E = {out.energy:.10f} (golden {want:.10f}, d {out.energy - want:.1e}) steps {out.cc['n_iter']}")
        assert abs(out.energy - want) < 1e-8, (line, out.energy, want)
        assert out.correlation_energy_cc == out.cc["E_corr"] and out.cc["converged"]
        text += log
    text = "\n".join(text)
    for s in ("Energy convergence tolerance:        0.0000000010", "Amplitude convergence tolerance:     0.0000000100",
              "Amplitude convergence tolerance:     0.0000000001", "Guess t-amplitude MP2 energy:", "Using DIIS, storing 6 matrices, for convergence.",
              "Using damping parameter of 0.30 for convergence.", "Starting CCD iterations...", "Starting LCCD iterations...",
              "Step          Correlation E               DE", "Connected doubles contribution:", "CCD correlation energy:", "LCCD correlation energy:",
              "Correlation energy from CCD:", "Correlation energy from LCCD:", "Final single point energy:"):
        assert s in text, s
    for line in ("SPE : O O 1.2075 : CCD STO-3G : ML 3", "SPE : O O 1.2075 : LCCD STO-3G : ML 3", "SPE : N N 1.0977 : UCCD STO-3G",
                 "SPE : N N 1.0977 : ULCCD STO-3G", "SPE : N N 1.0977 : CCD STO-3G : DIPOLE", "SPE : N N 1.0977 : LCCD STO-3G : POLAR",
                 "SPE : N N 1.0977 : CCD STO-3G : HYPER", "SPE : N N 1.0977 : CCSD STO-3G", "SPE : N N 1.0977 : CID STO-3G"):
        with pytest.raises(TunaError):
            run(line, engine=engine)
