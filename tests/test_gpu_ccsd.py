"""GPU: restricted LCCSD, QCISD and CCSD iterated on the resident tensor (tf_ccsd_rhf) against the reference program's own iteration
(tests/golden/ccsd_systems.npz) and the independent dense closed-shell iteration of tests/ccsd_reference.py: converged energies, the
energy of every step, the step count and the final t1; fixed numbers of steps element by element at the batch edges of the ladder; the
nesting with LCCD; the layouts against each other; repeatability, and that the doubles-only methods on the same context do not move;
refusals; the energy driver.  Tolerances are those of tests/test_gpu_ccd.py.  Every test hands the shared context back with the default
layout."""
import ctypes

import numpy as np
import pytest

import ccsd_reference as sr
import mp3_reference as mr
from test_ccd_reference import split
from test_gpu_ccd import LOOPS
from test_gpu_mp3 import SYSTEMS, _random_orbitals, _reset, _system
from tuna_amd._lib import CcOpts, CcsdResult, TunaError, ptr

pytestmark = pytest.mark.gpu

TF_EINVAL, TF_ENOTCONV = -1, -4
METHODS = ("LCCSD", "QCISD", "CCSD")
GOLD = dict(conv_delta_E=1e-11, conv_amplitudes=1e-10, use_diis=True, max_diis=6)     # the thresholds of tools/make_golden_ccsd.py


@pytest.fixture(scope="module")
def ccsd_golden(golden):
    return split(golden("ccsd_systems"))


@pytest.fixture(scope="module")
def mp3_golden(golden):
    return split(golden("mp3_systems"))


@pytest.fixture(scope="module")
def n2_tz():
    shells, aos = _system("n2_ccpvtz")
    return aos, mr.dense_eri(aos, shells)


def check_against_golden(r, g, pre, what, conv_delta_E=1e-11, conv_amplitudes=1e-10):
    """|E_corr - golden| < 1e-9; every step within 1e-8; max |t1 - golden t1| < 1e-8; step counts equal, or one apart where the golden's
    deciding ratio -- the largest of |dE|, ||dt2|| and ||dt1|| over their thresholds -- sits within a factor 2 of its threshold at the
    step where one side stopped"""
    want, dt2, dt1 = g[pre + "energies"], g[pre + "dt2_norms"], g[pre + "dt1_norms"]
    n, ng = r["n_iter"], int(g[pre + "n_iter"])
    m = min(n, ng)
    step_diff = np.abs(r["table"][:m, 1] - want[:m]).max()
    t1_diff = np.abs(r["t1"] - g[pre + "t1"]).max()
    print(f"\n[{what}] E_corr {r['E_corr']:.12f} golden {float(g[pre + 'E_corr']):.12f} d {r['E_corr'] - float(g[pre + 'E_corr']):.1e} steps {n} "
          f"golden {ng} max step d {step_diff:.1e} max t1 d {t1_diff:.1e} |t1| {r['t1_norm']:.6f}")
    assert r["converged"], what
    assert abs(r["E_corr"] - float(g[pre + "E_corr"])) < 1e-9, what
    assert step_diff < 1e-8, what
    assert t1_diff < 1e-8, what
    assert np.array_equal(r["table"][:, 0], np.arange(1, n + 1)) and np.allclose(np.diff(np.concatenate([[0.0], r["table"][:, 1]])), r["table"][:, 2],
                                                                               rtol=0, atol=1e-15)
    assert r["E_singles"] == 0.0 and r["E_corr"] == r["E_connected"] + r["E_disconnected"] and r["E_corr"] == r["table"][-1, 1]
    assert (r["E_disconnected"] == 0.0) == (not pre.startswith("CCSD")), what
    assert abs(r["E_disconnected"] - float(g[pre + "E_disconnected"])) < 1e-9 and abs(r["t1_norm"] - float(g[pre + "t1_norm"])) < 1e-8
    assert r["t1_norm"] == float(np.linalg.norm(r["t1"])) or abs(r["t1_norm"] - np.linalg.norm(r["t1"])) < 1e-15
    if n != ng:
        assert abs(n - ng) == 1, what
        k = min(n, ng) - 1                                                # the step at which one side stopped and the other went on
        dE = abs(want[k] - (want[k - 1] if k else 0.0))
        ratios = (dE / conv_delta_E, dt2[k] / conv_amplitudes, dt1[k] / conv_amplitudes)
        print(f"[{what}] step counts differ: golden ratios to the thresholds (|dE|, ||dt2||, ||dt1||) {ratios} at step {k + 1}")
        assert 0.5 < max(ratios) < 2.0, (what, ratios)


@pytest.mark.parametrize("tag", ["n2_ccpvdz", "n2_ccpvtz", "co_631g", "hf_ccpvdz", "ne_ccpvdz"])
def test_reference_orbitals_against_goldens(engine, ccsd_golden, mp3_golden, tag):
    g, m = ccsd_golden[tag], mp3_golden[tag]
    engine.set_basis(_system(tag)[1]).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed"
    nocc = int(m["n_occ"])
    for nf in (0, 1):
        m2 = engine.mp2_rhf(m["C"], m["eps"], nocc, nf)
        o = nocc - nf
        for method in METHODS:
            r = engine.ccsd_rhf(m["C"], m["eps"], nocc, nf, method=method, return_t1=True, **GOLD)
            check_against_golden(r, g, f"{method}_fc{nf}_", f"{tag} {method} fc{nf}")
            rel = abs(r["E_MP2"] - m2["E_MP2"]) / abs(m2["E_MP2"])
            print(f"[{tag} {method} fc{nf}] E_MP2 {r['E_MP2']:.12f} mp2_rhf {m2['E_MP2']:.12f} rel {rel:.1e} seconds {r['seconds']}")
            assert rel < 1e-12
            assert r["ladder_batches"] == r["n_iter"] * -(-o * o // 64)
            assert r["T1_diagnostic"] == r["t1_norm"] / np.sqrt(2.0 * o)


def test_golden_file_holds_the_required_systems(ccsd_golden):
    assert {"n2_ccpvdz", "n2_ccpvtz", "hf_ccpvdz", "ne_ccpvdz"} <= set(ccsd_golden) <= set(SYSTEMS)
    for g in ccsd_golden.values():
        for method in METHODS:
            assert f"{method}_fc0_E_corr" in g and f"{method}_fc1_t1" in g


def test_diis_nodiis_and_damping(engine, ccsd_golden, mp3_golden):
    g, m = ccsd_golden["n2_ccpvdz"], mp3_golden["n2_ccpvdz"]
    engine.set_basis(_system("n2_ccpvdz")[1]).build_eri(True)
    for method in METHODS:
        with_diis = engine.ccsd_rhf(m["C"], m["eps"], 7, 0, method=method, return_t1=True, **GOLD)
        plain = engine.ccsd_rhf(m["C"], m["eps"], 7, 0, method=method, return_t1=True, **dict(GOLD, use_diis=False))
        damped = engine.ccsd_rhf(m["C"], m["eps"], 7, 0, method=method, return_t1=True, damping=0.3, **GOLD)
        check_against_golden(plain, g, f"{method}_nodiis_", f"{method} NODIIS")
        check_against_golden(damped, g, f"{method}_damp03_", f"{method} CORRDAMP 0.3")
        assert plain["n_iter"] >= with_diis["n_iter"]


@pytest.mark.parametrize("width", [1, 7, 8, 12])
def test_fixed_steps_against_the_independent_checker(engine, n2_tz, width):
    """N2/cc-pVTZ, random orthonormal orbitals: one pair; 49 pairs (one partial batch of the ladder); 64 pairs (one full batch); 144 pairs
    (three batches, the last one partial).  The loops of tests/test_gpu_ccd.py for the three methods, element by element."""
    aos, E = n2_tz
    engine.set_basis(aos).build_eri(True)
    C, eps = _random_orbitals(engine.N, 30 + width)
    Co, Cv, eo, ev = mr._windows(C, eps, width, 0)
    blocks = (mr.mo_tensor(E, Co, Cv, Co, Cv), mr.mo_tensor(E, Co, Co, Cv, Cv), mr.mo_tensor(E, Co, Co, Co, Co), mr.mo_tensor(E, Co, Co, Co, Cv),
              mr.mo_tensor(E, Co, Cv, Cv, Cv), mr.mo_tensor(E, Cv, Cv, Cv, Cv))          # once, shared by every loop and method
    t0 = blocks[0].transpose(0, 2, 1, 3) / sr._denominators(eo, ev)
    bad = []
    for method in METHODS:
        step = sr.restricted_step(*blocks, eo, ev, method)
        for what, (k, gpu_loop, ref_loop) in LOOPS.items():
            r = engine.ccsd_rhf(C, eps, width, 0, method=method, max_iter=k, conv_delta_E=0.0, conv_amplitudes=0.0, return_t1=True, return_t2=True,
                                allow_unconverged=True, **gpu_loop)
            ref = sr._run(step, sr._energy_parts(blocks[0]), t0, (width, len(ev)), method, k, **ref_loop)
            s2, s1 = np.abs(ref["t2"]).max(), np.abs(ref["t1"]).max()
            d2, d1 = np.abs(r["t2"] - ref["t2"]).max() / s2, np.abs(r["t1"] - ref["t1"]).max() / s1
            dE = np.abs(r["table"][:, 1] - np.array(ref["energies"])) / np.abs(ref["energies"])
            print(f"\n[width {width} {method}, {what}] max|t2| {s2:.3f} max|t1| {s1:.3f} max|dt2|/max|t2| {d2:.1e} max|dt1|/max|t1| {d1:.1e} "
                  f"rel dE per step {dE} E {ref['energies']}")
            assert s2 < 1.0 and 0.0 < s1 < 1.0 and r["n_iter"] == k and not r["converged"]
            if not (d2 <= 1e-10 and d1 <= 1e-10 and np.all(dE <= 1e-11)):
                bad.append((method, what, d2, d1, dE))
            assert np.array_equal(r["t2"], r["t2"].transpose(1, 0, 3, 2))
            assert r["ladder_batches"] == k * -(-width * width // 64)
    assert not bad, bad


def test_small_diis_depths(engine, mp3_golden):
    """tests/test_gpu_ccd.py's test of the same name for LCCSD and CCSD: N2/cc-pVDZ, golden orbitals, packed layout, ten fixed steps with
    damping 0.2 at max_diis 1, 2 and 3 (a vector leaves the history in every step from the third on), t1 and t2 element by element against
    the checker's loop at the same depth; depths 1 and 2 bit for bit.  At these settings the checker's two closed-shell forms
    (restricted_iterations, iterations_from_blocks) agree over the ten steps to 3.5e-15 in t2 / max|t2|, 5.0e-15 in t1 / max|t1| and
    3.7e-16 in E (max|t2| = 0.079, max|t1| = 0.023), so the tolerances are five orders above the checker's own noise.  (Its spin-orbital
    form is no yardstick here: with DIIS on, its error dots run over the spin-orbital amplitudes, another metric, and its path leaves
    the closed-shell one at the first extrapolation.)"""
    m = mp3_golden["n2_ccpvdz"]
    shells, aos = _system("n2_ccpvdz")
    E = mr.dense_eri(aos, shells)
    engine.set_basis(aos).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed"
    C, eps = m["C"], m["eps"]
    Co, Cv, eo, ev = mr._windows(C, eps, 7, 0)
    blocks = (mr.mo_tensor(E, Co, Cv, Co, Cv), mr.mo_tensor(E, Co, Co, Cv, Cv), mr.mo_tensor(E, Co, Co, Co, Co), mr.mo_tensor(E, Co, Co, Co, Cv),
              mr.mo_tensor(E, Co, Cv, Cv, Cv), mr.mo_tensor(E, Cv, Cv, Cv, Cv))          # once: sr.restricted_iterations makes the same six
    t0 = blocks[0].transpose(0, 2, 1, 3) / sr._denominators(eo, ev)
    bad = []
    for method in ("LCCSD", "CCSD"):
        step = sr.restricted_step(*blocks, eo, ev, method)
        runs = {}
        for depth in (1, 2, 3):
            r = engine.ccsd_rhf(C, eps, 7, 0, method=method, max_iter=10, conv_delta_E=0.0, conv_amplitudes=0.0, return_t1=True, return_t2=True,
                                allow_unconverged=True, use_diis=True, max_diis=depth, damping=0.2)
            ref = sr._run(step, sr._energy_parts(blocks[0]), t0, (7, len(ev)), method, 10, diis=True, max_diis=depth, damping=0.2)
            s2, s1 = np.abs(ref["t2"]).max(), np.abs(ref["t1"]).max()
            d2, d1 = np.abs(r["t2"] - ref["t2"]).max() / s2, np.abs(r["t1"] - ref["t1"]).max() / s1
            dE = np.abs(r["table"][:, 1] - np.array(ref["energies"])) / np.abs(ref["energies"])
            print(f"\n[{method}, max_diis {depth}] max|t2| {s2:.3f} max|t1| {s1:.4f} max|dt2|/max|t2| {d2:.1e} max|dt1|/max|t1| {d1:.1e} rel dE per step {dE}")
            assert s2 < 1.0 and 0.0 < s1 < 1.0 and r["n_iter"] == 10 and not r["converged"]
            if not (d2 <= 1e-10 and d1 <= 1e-10 and np.all(dE <= 1e-11)):
                bad.append((method, depth, d2, d1, dE))
            runs[depth] = r
        for key in ("t1", "t2", "table"):
            assert np.array_equal(runs[1][key], runs[2][key]), (method, key)
        assert not np.array_equal(runs[2]["t2"], runs[3]["t2"]), method      # (the depth does reach the loop)
    assert not bad, bad


def test_nesting_with_lccd(engine, mp3_golden, n2_tz):
    """t1 = 0 goes in, so the doubles of LCCSD's first step see no singles: LCCD's first step; its singles come out nonzero"""
    m = mp3_golden["n2_ccpvtz"]
    engine.set_basis(n2_tz[0]).build_eri(True)
    for nf in (0, 1):
        r = engine.ccsd_rhf(m["C"], m["eps"], 7, nf, method="LCCSD", max_iter=1, return_t1=True, allow_unconverged=True)
        d = engine.ccd_rhf(m["C"], m["eps"], 7, nf, method="LCCD", max_iter=1, allow_unconverged=True)
        rel = abs(r["E_corr"] - d["E_corr"]) / abs(d["E_corr"])
        print(f"\n[N2/cc-pVTZ fc{nf}] LCCSD step 1 {r['E_corr']:.13f} LCCD step 1 {d['E_corr']:.13f} rel {rel:.1e} |t1| {r['t1_norm']:.6f}")
        assert r["n_iter"] == 1 and not r["converged"] and rel < 1e-11
        assert r["t1_norm"] > 1e-3 and np.abs(r["t1"]).max() > 1e-4


def test_layouts_agree(engine, mp3_golden, n2_tz):
    m = mp3_golden["n2_ccpvtz"]
    try:
        e = {}
        for layout in ("packed", "rows", "tiles"):
            engine.set_basis(n2_tz[0]).build_eri(True, layout=layout)
            assert engine.eri_storage()["layout"] == layout
            e[layout] = {method: engine.ccsd_rhf(m["C"], m["eps"], 7, 1, method=method, return_t1=True, **GOLD) for method in METHODS}
        for method in METHODS:
            for lt in ("rows", "tiles"):
                d = abs(e[lt][method]["E_corr"] - e["packed"][method]["E_corr"])
                d1 = np.abs(e[lt][method]["t1"] - e["packed"][method]["t1"]).max()
                print(f"\n[{method}] {lt} - packed {d:.1e} t1 {d1:.1e} steps {e[lt][method]['n_iter']} / {e['packed'][method]['n_iter']}")
                assert d < 1e-10 and d1 < 1e-10 and e[lt][method]["converged"]
    finally:
        _reset(engine)
    engine.set_basis(n2_tz[0]).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed"


def test_repeatable_and_the_doubles_methods_do_not_move(engine, mp3_golden):
    m = mp3_golden["n2_ccpvdz"]
    engine.set_basis(_system("n2_ccpvdz")[1]).build_eri(True)

    def others():
        r3, r4 = engine.mp3_rhf(m["C"], m["eps"], 7, 0), engine.mp4_rhf(m["C"], m["eps"], 7, 0, level="SDQ")
        cc = [engine.ccd_rhf(m["C"], m["eps"], 7, 0, method=x, return_t2=True, **GOLD) for x in ("LCCD", "CCD")]
        return ([r3[k] for k in ("E_OS", "E_SS", "E_pp", "E_hh", "E_ring")], [r4[k] for k in ("E_MP2", "E_MP3", "E_S", "E_D", "E_Q")],
                [(c["E_corr"], c["n_iter"], c["table"].tobytes(), c["t2"].tobytes()) for c in cc])
    before = others()
    for method in METHODS:
        a, b = (engine.ccsd_rhf(m["C"], m["eps"], 7, 0, method=method, return_t1=True, return_t2=True, damping=0.1, **GOLD) for _ in range(2))
        assert a["n_iter"] == b["n_iter"] and np.array_equal(a["table"], b["table"])
        assert np.array_equal(a["t1"], b["t1"]) and np.array_equal(a["t2"], b["t2"])
        assert a["E_corr"] == b["E_corr"] and a["E_MP2"] == b["E_MP2"] and a["t1_norm"] == b["t1_norm"] and a["E_disconnected"] == b["E_disconnected"]
    assert others() == before


def test_refusals(engine, ccsd_golden, mp3_golden):
    from tuna_amd.engine import Engine
    g, m = ccsd_golden["n2_ccpvdz"], mp3_golden["n2_ccpvdz"]
    shells, aos = _system("n2_ccpvdz")
    engine.set_basis(aos).build_eri(True)
    first = engine.ccsd_rhf(m["C"], m["eps"], 7, 0, method="CCSD", **GOLD)
    L, ctx, N = engine._L, engine._ctx, engine.N
    C, eps = (np.ascontiguousarray(x, dtype=np.float64) for x in (m["C"], m["eps"]))

    def opts(method=2, max_iter=100):
        return CcOpts(method, max_iter, 1, 6, 1e-11, 1e-10, 0.0)
    res = CcsdResult()
    good, po, pr = opts(), ctypes.byref, ctypes.byref(res)
    bad = [(po(good), 7, -1, ptr(C), ptr(eps), pr), (po(good), 7, 7, ptr(C), ptr(eps), pr), (po(good), 0, 0, ptr(C), ptr(eps), pr),
           (po(good), N, 0, ptr(C), ptr(eps), pr), (None, 7, 0, ptr(C), ptr(eps), pr), (po(good), 7, 0, None, ptr(eps), pr),
           (po(good), 7, 0, ptr(C), None, pr), (po(good), 7, 0, ptr(C), ptr(eps), None), (po(opts(max_iter=0)), 7, 0, ptr(C), ptr(eps), pr),
           (po(opts(method=3)), 7, 0, ptr(C), ptr(eps), pr), (po(opts(method=-1)), 7, 0, ptr(C), ptr(eps), pr)]
    for args in bad:
        assert L.tf_ccsd_rhf(ctx, *args) == TF_EINVAL, args
        again = engine.ccsd_rhf(m["C"], m["eps"], 7, 0, method="CCSD", **GOLD)          # the context stays usable
        assert again["E_corr"] == first["E_corr"] and again["n_iter"] == first["n_iter"]
    assert L.tf_ccsd_rhf(None, po(good), 7, 0, ptr(C), ptr(eps), pr) == TF_EINVAL
    with Engine(0) as fresh:                                          # no tensor yet
        fresh.set_basis(aos)
        assert fresh._L.tf_ccsd_rhf(fresh._ctx, po(good), 7, 0, ptr(C), ptr(eps), pr) == TF_EINVAL
    with Engine(0, 0, 2) as half:                                     # rank 0 of two: sharding is not supported
        half.set_basis(aos).build_eri(True)
        assert half._L.tf_ccsd_rhf(half._ctx, po(good), 7, 0, ptr(C), ptr(eps), pr) == TF_EINVAL
    with pytest.raises(TunaError):
        engine.ccsd_rhf(m["C"], m["eps"], 7, 0, method="CCD")
    with pytest.raises(TunaError):
        engine.ccd_rhf(m["C"], m["eps"], 7, 0, method="CCSD")
    # two steps at tight thresholds: not converged, the outputs hold the second step
    table, t1 = np.zeros((2, 3)), np.zeros((7, N - 7))
    res2 = CcsdResult()
    res2.table, res2.t1 = ptr(table), ptr(t1)
    assert L.tf_ccsd_rhf(ctx, po(opts(max_iter=2)), 7, 0, ptr(C), ptr(eps), ctypes.byref(res2)) == TF_ENOTCONV
    assert res2.n_iter == 2 and not res2.converged and res2.e_corr == table[1, 1] and np.all(table[:, 0] == [1, 2])
    assert res2.e_corr == res2.e_connected + res2.e_disconnected and res2.ladder_batches == 2
    assert np.abs(table[:, 1] - g["CCSD_fc0_energies"][:2]).max() < 1e-8
    assert res2.t1_norm > 0.0 and abs(res2.t1_norm - np.linalg.norm(t1)) < 1e-15
    with pytest.raises(TunaError) as e:
        engine.ccsd_rhf(m["C"], m["eps"], 7, 0, method="CCSD", max_iter=2, **GOLD)
    assert e.value.code == TF_ENOTCONV
    r = engine.ccsd_rhf(m["C"], m["eps"], 7, 0, method="CCSD", max_iter=2, return_t1=True, allow_unconverged=True, **GOLD)
    assert r["n_iter"] == 2 and not r["converged"] and np.array_equal(r["table"], table) and np.array_equal(r["t1"], t1)
    again = engine.ccsd_rhf(m["C"], m["eps"], 7, 0, method="CCSD", **GOLD)
    assert again["E_corr"] == first["E_corr"] and abs(again["E_corr"] - float(g["CCSD_fc0_E_corr"])) < 1e-9
    assert engine.eri_storage()["layout"] == "packed"


def test_energy_driver(engine, ccsd_golden, mp3_golden):
    """calculate_energy with a Calculation that names the method (the input line does not route these names yet)"""
    from tuna_amd import energy
    g, E_SCF = ccsd_golden["n2_ccpvdz"], float(mp3_golden["n2_ccpvdz"]["E_SCF"])
    _, _, basis, symbols, R, params = energy.parse_input("SPE : N N 1.0977 : HF CC-PVDZ : TIGHT")
    text = []
    for method in METHODS:
        calc = energy.interpret_keywords(params, energy.Calculation("SPE", "HF", basis))
        calc.coupled_cluster = method
        log = []
        out = energy.calculate_energy(symbols, R, calc, engine, False, log.append)
        want = E_SCF + float(g[f"{method}_fc0_E_corr"])
        print(f"\n[{method}] E = {out.energy:.10f} (golden {want:.10f}, d {out.energy - want:.1e}) steps {out.cc['n_iter']}")
        assert abs(out.energy - want) < 1e-8, (method, out.energy, want)
        assert out.correlation_energy_cc == out.cc["E_corr"] and out.cc["converged"]
        text += log
    text = "\n".join(text)
    for s in ("Energy convergence tolerance:        0.0000000010", "Amplitude convergence tolerance:     0.0000000100",
              "Guess t-amplitude MP2 energy:", "Using DIIS, storing 6 matrices, for convergence.", "Starting CCSD iterations...",
              "Starting QCISD iterations...", "Starting LCCSD iterations...", "Step          Correlation E               DE",
              "Singles contribution:                0.0000000000", "Connected doubles contribution:", "Disconnected doubles contribution:   0.0000000000",
              "CCSD correlation energy:", "QCISD correlation energy:", "LCCSD correlation energy:",
              "Norm of singles amplitudes:", "Value of T1 diagnostic:", "Correlation energy from CCSD:", "Correlation energy from QCISD:",
              "Correlation energy from LCCSD:", "Final single point energy:"):
        assert s in text, s
    with pytest.raises(TunaError, match="is not supported"):
        energy.run("SPE : N N 1.0977 : CCSD STO-3G", engine=engine)
