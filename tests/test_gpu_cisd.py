"""GPU: CIS(D) on the resident tensor (tf_cis_d_rhf: the dressed AO->MO transformation, the operand and direct kernels of
tf_cisd.hip.h, the rocBLAS products of the indirect part) against the reference program's own corrections
(tests/golden/cisd_systems.npz, cisd_text.json) and the independent spin-orbital NumPy checker of tests/cisd_reference.py: every
stored state of every system, frozen 0 and 1; batches against single states and a second call bit for bit; the direct and indirect
parts and the smallest denominator; o = v = 1, o = 1, an atom, ragged 16-wide tiles (v = 53), a state with one non-zero amplitude;
the three layouts and the expanded-block transformation; the refusals of the raw ABI; the energy driver and the input line.  Every test
hands the shared context back with the default layout.

Measured on one MI355X over all 114 stored states: the largest |E_D - golden| is 4.2e-16 Eh (HF/cc-pVDZ; the same on the rows and tiles
layouts and with TF_MO_Q1=0: at most 2.6e-16 Eh for CO/6-31G); the parts against the NumPy checker, relative to the sum of the magnitudes
of the part's terms (plus the S_FLOOR of the CPU test), at most 2.2e-15 over the stored states, 3.3e-15 for the unit vectors and 1.3e-14
for H2/cc-pVDZ (direct part, whose scale is the smallest).  DEVICE_TOL and SPLIT_TOL are ten times the largest of each: the margin covers
rocBLAS differences between machines."""
import ctypes
import json
import os

import numpy as np
import pytest

import cisd_reference as cd
from conftest import GOLD, R_H2
from test_cis_reference import SYSTEMS, split, system
from test_cisd_reference import S_FLOOR, runs
from test_gpu_mp3 import _reset
from tuna_amd import energy
from tuna_amd import molecule as mol
from tuna_amd._lib import CisDResult, TunaError, ptr

pytestmark = pytest.mark.gpu

TF_EINVAL = -1
MEASURED_GOLDEN, MEASURED_SPLIT = 4.2e-16, 1.3e-14
DEVICE_TOL = 10 * MEASURED_GOLDEN     # Eh per state
SPLIT_TOL = 10 * MEASURED_SPLIT       # per part, relative to the sum of the magnitudes of its terms
assert DEVICE_TOL <= 1e-11            # the loosest energy parity with the reference that the project documents (UMP2)


@pytest.fixture(scope="module")
def goldens(golden):
    return split(golden("cis_systems")), split(golden("cisd_systems"))


def stored(d, pre):
    return d[pre + "b"], d[pre + "omega"], d[pre + "triplet"], d[pre + "E_D"], d[pre + "min_denominator"]


def same_bits(a, b, which=None):
    return all(np.array_equal(a[k] if which is None else a[k][which], b[k]) for k in ("E_D", "E_direct", "E_indirect", "min_denominator"))


@pytest.mark.parametrize("tag", list(SYSTEMS))
def test_golden_parity(engine, goldens, tag):
    """Every stored state of the system, frozen 0 and 1, CIS and (CO/6-31G) TDHF with b = X + Y, in one call per run: E_D against the
    reference program's, e_d = e_direct + e_indirect exactly, min |D + omega| against the generator's.  The systems cover o = v = 1
    (H2/STO-3G), an atom (Ne), v = 53 = three 16-wide tiles and a ragged fourth (N2/cc-pVTZ), and o even and odd (frozen 0 and 1)."""
    gc, gd = goldens
    g, d = gc[tag], gd[tag]
    engine.set_basis(system(tag)[1]).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed"
    bad = []
    for method, nf in runs(d):
        pre = f"{method}_fc{nf}_"
        b, w, flags, E_D, dmin = stored(d, pre)
        r = engine.cis_d_rhf(g["C"], g["eps"], int(g["n_occ"]), nf, b=b, omega=w, triplet=flags)
        dE = np.abs(r["E_D"] - E_D).max()
        dm = np.abs(r["min_denominator"] / dmin - 1).max()
        print(f"\n[{tag} {pre}] {len(w)} states max |dE_D| {dE:.1e} (tol {DEVICE_TOL:.1e}) min denominator rel d {dm:.1e} seconds {r['seconds']}")
        assert np.array_equal(r["E_D"], r["E_direct"] + r["E_indirect"])
        if not (dE < DEVICE_TOL and dm < 1e-13):
            bad.append((pre, dE, dm))
    assert not bad, bad


def test_batches_and_a_second_call_give_the_same_bits(engine, goldens):
    """N2/cc-pVDZ, frozen 1 (o = 6, v = 21: two tiles per edge, the second ragged), the eight stored states: all in one call, one call per
    state, singlets and triplets interleaved in another order, and the first call again: every state's E_D, E_direct, E_indirect and
    min_denominator are the same to the last bit."""
    gc, gd = goldens
    g, d = gc["n2_ccpvdz"], gd["n2_ccpvdz"]
    engine.set_basis(system("n2_ccpvdz")[1]).build_eri(True)
    b, w, flags, _, _ = stored(d, "CIS_fc1_")
    args = (g["C"], g["eps"], 7, 1)
    one_call = engine.cis_d_rhf(*args, b=b, omega=w, triplet=flags)
    assert same_bits(one_call, engine.cis_d_rhf(*args, b=b, omega=w, triplet=flags))
    for n in range(len(w)):
        assert same_bits(one_call, engine.cis_d_rhf(*args, b=b[n], omega=w[n], triplet=flags[n]), slice(n, n + 1)), n
    singlets, triplets = np.flatnonzero(flags == 0), np.flatnonzero(flags == 1)
    order = np.array([k for pair in zip(singlets[::-1], triplets) for k in pair])
    assert len(order) == len(w) and list(flags[order][:4]) == [0, 1, 0, 1]
    assert same_bits(one_call, engine.cis_d_rhf(*args, b=b[order], omega=w[order], triplet=flags[order]), order)


SPLIT_CASES = [("h2_sto3g", 0, None), ("ne_ccpvdz", 1, None), ("co_631g", 0, None), ("hf_ccpvdz", 1, None), ("n2_ccpvtz", 0, 1)]


@pytest.mark.parametrize("tag,nf,first", SPLIT_CASES)
def test_parts_against_the_independent_checker(engine, goldens, tag, nf, first):
    """E_direct, E_indirect and min |D + omega| of the stored CIS states (N2/cc-pVTZ: the first singlet and the first triplet) against
    the spin-orbital NumPy expressions, each part relative to the sum of the magnitudes of its terms."""
    gc, gd = goldens
    g, d = gc[tag], gd[tag]
    shells, aos = system(tag)
    engine.set_basis(aos).build_eri(True)
    b, w, flags, _, _ = stored(d, f"CIS_fc{nf}_")
    if first:
        keep = [int(np.flatnonzero(flags == 0)[0]), int(np.flatnonzero(flags == 1)[0])]
        b, w, flags = b[keep], w[keep], flags[keep]
    nocc = int(g["n_occ"])
    prep = cd.prepare(cd.dense_eri(aos, shells), g["C"], g["eps"], nocc, nf)
    r = engine.cis_d_rhf(g["C"], g["eps"], nocc, nf, b=b, omega=w, triplet=flags)
    worst = np.zeros(3)
    for n in range(len(w)):
        ref = cd.correction(prep, b[n], float(w[n]), int(flags[n]))
        worst = np.maximum(worst, [abs(r["E_direct"][n] - ref["E_direct"]) / (ref["S_direct"] + S_FLOOR),
                                   abs(r["E_indirect"][n] - ref["E_indirect"]) / (ref["S_indirect"] + S_FLOOR),
                                   abs(r["min_denominator"][n] / ref["min_denominator"] - 1)])
    print(f"\n[{tag} fc{nf}] {len(w)} states: direct {worst[0]:.1e} indirect {worst[1]:.1e} (tol {SPLIT_TOL:.1e}) min denominator rel d {worst[2]:.1e}")
    assert worst[0] < SPLIT_TOL and worst[1] < SPLIT_TOL and worst[2] < 1e-13


def test_one_occupied_orbital_and_one_amplitude(engine, goldens):
    """H2/cc-pVDZ (o = 1, v = 9, one ragged tile; orbitals of the CPU oracle's RHF, the three lowest states of either multiplicity from
    tf_cis_rhf on them), and CO/6-31G with b a single non-zero amplitude (one column of the dressed orbitals, one row of the (ki|jb)
    product; first and last (i, a), both multiplicities, omega = 0.3 Eh): E_D and its parts against the spin-orbital NumPy expressions."""
    from oracle import scf_oracle as so
    atoms = mol.make_atoms(["H", "H"], R_H2)
    shells = mol.build_shells(atoms, "cc-pVDZ")
    aos = mol.expand_cartesian_aos(shells)
    engine.set_basis(aos).build_eri(True)
    E = cd.dense_eri(aos, shells)
    S, T, V, _, _ = engine.one_electron([a.origin for a in atoms], [float(a.charge) for a in atoms], [0.0, 0.0, 0.0])
    X, _, _ = so.orthogonaliser(S)
    P0, E0 = so.core_guess(T, V, X, 1)
    scf = so.run_rhf(S, T, V, E, X, P0, E0, 1, mol.nuclear_repulsion(atoms), [5, 5], conv="extreme", damping=False)
    C, eps = scf["C"], scf["epsilons"]
    assert engine.N == 10
    cis = engine.cis_rhf(C, eps, 1, 0, method="CIS", n_keep=3)
    b = np.concatenate([cis["X_singlet"], cis["X_triplet"]])
    w = np.concatenate([cis["E_singlet"][:3], cis["E_triplet"][:3]])
    flags = np.array([0, 0, 0, 1, 1, 1])
    cases = [("H2/cc-pVDZ", E, C, eps, 1, b, w, flags)]
    gc, _ = goldens
    g = gc["co_631g"]
    shells_co, aos_co = system("co_631g")
    o, v = 7, 11
    units = np.zeros((4, o, v))
    units[0, 0, 0] = units[1, 0, 0] = units[2, o - 1, v - 1] = units[3, o - 1, v - 1] = 1.0
    gaps = np.full(4, 0.3)                                        # (any energy away from a resonance: D_ijab <= -1.4 Eh here)
    cases.append(("CO/6-31G unit vectors", cd.dense_eri(aos_co, shells_co), g["C"], g["eps"], 7, units, gaps, np.array([0, 1, 0, 1])))
    for name, E, C, eps, nocc, b, w, flags in cases:
        if name.startswith("CO"):
            engine.set_basis(aos_co).build_eri(True)
        prep = cd.prepare(E, C, eps, nocc, 0)
        r = engine.cis_d_rhf(C, eps, nocc, 0, b=b, omega=w, triplet=flags)
        worst = np.zeros(3)
        for n in range(len(w)):
            ref = cd.correction(prep, b[n], float(w[n]), int(flags[n]))
            assert ref["min_denominator"] > 0.1
            worst = np.maximum(worst, [abs(r["E_D"][n] - ref["E_D"]), abs(r["E_direct"][n] - ref["E_direct"]) / (ref["S_direct"] + S_FLOOR),
                                       abs(r["E_indirect"][n] - ref["E_indirect"]) / (ref["S_indirect"] + S_FLOOR)])
        print(f"\n[{name}] {len(w)} states: max |dE_D| {worst[0]:.1e} direct {worst[1]:.1e} indirect {worst[2]:.1e} E_D {r['E_D']}")
        assert worst[0] < DEVICE_TOL and worst[1] < SPLIT_TOL and worst[2] < SPLIT_TOL


def test_layouts_and_the_expanded_block_transformation(engine, goldens, monkeypatch):
    """CO/6-31G, CIS and TDHF states, on the packed, rows and tiles layouts and on packed with TF_MO_Q1=0 (the transformation without the
    hand-written first quarter): the same golden numbers within the same tolerance."""
    gc, gd = goldens
    g, d = gc["co_631g"], gd["co_631g"]
    aos = system("co_631g")[1]
    monkeypatch.delenv("TF_MO_Q1", raising=False)
    try:
        for layout, q1 in (("packed", None), ("packed", "0"), ("rows", None), ("tiles", None)):
            engine.set_basis(aos).build_eri(True, layout=layout)
            assert engine.eri_storage()["layout"] == layout
            if q1:
                monkeypatch.setenv("TF_MO_Q1", q1)
            for pre in ("CIS_fc1_", "TDHF_fc0_"):
                b, w, flags, E_D, dmin = stored(d, pre)
                r = engine.cis_d_rhf(g["C"], g["eps"], 7, int(pre[-2]), b=b, omega=w, triplet=flags)
                dE = np.abs(r["E_D"] - E_D).max()
                print(f"\n[{layout}{' TF_MO_Q1=0' if q1 else ''} {pre}] max |dE_D| {dE:.1e}")
                assert dE < DEVICE_TOL and np.abs(r["min_denominator"] / dmin - 1).max() < 1e-13
            monkeypatch.delenv("TF_MO_Q1", raising=False)
    finally:
        monkeypatch.delenv("TF_MO_Q1", raising=False)
        _reset(engine)
    engine.set_basis(aos).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed"


def test_refusals(engine, goldens):
    """Every TF_EINVAL case of the header through the raw ABI, each followed by a good call on the same context with the first call's bits."""
    from tuna_amd.engine import Engine
    gc, gd = goldens
    g, d = gc["hf_ccpvdz"], gd["hf_ccpvdz"]
    aos = system("hf_ccpvdz")[1]
    engine.set_basis(aos).build_eri(True)
    nocc, N = 5, engine.N
    b, w, flags, E_D, _ = stored(d, "CIS_fc0_")
    b, w, flags = b[:2], w[:2], flags[:2]
    first = engine.cis_d_rhf(g["C"], g["eps"], nocc, 0, b=b, omega=w, triplet=flags)
    L, ctx = engine._L, engine._ctx
    C, eps, bb, ww = (np.ascontiguousarray(x, dtype=np.float64) for x in (g["C"], g["eps"], b, w))
    ff, two, neg = (np.ascontiguousarray(x, dtype=np.int32) for x in (flags, [0, 2], [-1, 0]))
    e = [np.zeros(2) for _ in range(4)]

    def result(skip=None):
        res = CisDResult()
        for k, name in enumerate(("e_d", "e_direct", "e_indirect", "min_denominator")):
            if name != skip:
                setattr(res, name, ptr(e[k]))
        return res
    ok = result()
    pr = ctypes.byref(ok)
    good = (nocc, 0, ptr(C), ptr(eps), 2, ptr(bb), ptr(ww), ptr(ff), pr)
    bad = [(nocc, -1) + good[2:], (nocc, nocc) + good[2:], (0, 0) + good[2:], (N, 0) + good[2:],
           good[:2] + (None,) + good[3:], good[:3] + (None,) + good[4:], good[:4] + (0,) + good[5:], good[:4] + (-3,) + good[5:],
           good[:5] + (None,) + good[6:], good[:6] + (None,) + good[7:], good[:7] + (None,) + good[8:], good[:8] + (None,),
           good[:7] + (ptr(two), pr), good[:7] + (ptr(neg), pr)] + [good[:8] + (ctypes.byref(result(skip)),) for skip in ("e_d", "e_direct", "e_indirect")]
    for args in bad:
        assert L.tf_cis_d_rhf(ctx, *args) == TF_EINVAL, args
        assert "tf_cis_d_rhf" in L.tf_last_error(ctx).decode()
        assert same_bits(first, engine.cis_d_rhf(g["C"], g["eps"], nocc, 0, b=b, omega=w, triplet=flags))      # the context stays usable
    assert L.tf_cis_d_rhf(None, *good) == TF_EINVAL
    with Engine(0) as fresh:                                          # no tensor yet
        fresh.set_basis(aos)
        assert fresh._L.tf_cis_d_rhf(fresh._ctx, *good) == TF_EINVAL and "tf_build_eri" in fresh._L.tf_last_error(fresh._ctx).decode()
    with Engine(0, 0, 2) as half:                                     # rank 0 of two: sharding is not supported
        half.set_basis(aos).build_eri(True)
        assert half._L.tf_cis_d_rhf(half._ctx, *good) == TF_EINVAL and "world > 1" in half._L.tf_last_error(half._ctx).decode()
    # a good call through the bare ABI, and one without min_denominator
    assert L.tf_cis_d_rhf(ctx, *good) == 0
    assert all(np.array_equal(e[k], first[name]) for k, name in enumerate(("E_D", "E_direct", "E_indirect", "min_denominator")))
    e[3][:] = -1.0
    assert L.tf_cis_d_rhf(ctx, *(good[:8] + (ctypes.byref(result("min_denominator")),))) == 0
    assert np.array_equal(e[0], first["E_D"]) and np.all(e[3] == -1.0)
    with pytest.raises(TunaError, match=r"b must be \[n_states, 5, 14\]"):
        engine.cis_d_rhf(g["C"], g["eps"], nocc, 0, b=np.zeros((2, 5, 13)), omega=w, triplet=flags)
    assert engine.eri_storage()["layout"] == "packed"


def test_energy_driver_and_the_input_line(engine, goldens):
    """calculate_energy with do_perturbative_doubles for CO/6-31G, CIS root 1 and TDHF root 1, and the input line with the keyword:
    out.energy against E_SCF + omega + E_D of the golden file within the 1e-8 Eh of the project's input-line tests, and the printed
    section against the reference's.  Root 1 of CO is one component of a 3-Pi pair, and E_D is the same for any rotation within a
    symmetry-degenerate pair (both components have the same stored E_D), so the device's own eigenvector is a fair input although it
    need not be the golden's."""
    with open(os.path.join(GOLD, "cisd_text.json")) as f:
        texts = {t["method"]: t for t in json.load(f)}
    _, gd = goldens
    d = gd["co_631g"]
    for method in ("CIS", "TDHF"):
        assert abs(d[f"{method}_fc0_E_D"][0] - d[f"{method}_fc0_E_D"][1]) < 1e-13 and abs(d[f"{method}_fc0_omega"][0] - d[f"{method}_fc0_omega"][1]) < 1e-12
    runs_ = []
    for method in ("CIS", "TDHF"):
        calc = energy.interpret_keywords(["EXTREME"], energy.Calculation("SPE", "HF", "6-31G"))
        calc.excited_state, calc.tamm_dancoff_approximation, calc.do_perturbative_doubles = method, method == "CIS", True
        log = []
        runs_.append((method, energy.calculate_energy(["C", "O"], mol.angstrom_to_bohr(1.128), calc, engine, False, log.append), log))
    log = []
    runs_.append(("CIS", energy.run("SPE : C O 1.128 : CIS 6-31G : (D) EXTREME", silent=False, engine=engine, log=log.append), log))
    for method, out, log in runs_:
        t = texts[method]
        want = t["E_SCF"] + t["omega"] + t["E_D"]
        ex = out.excited
        print(f"\n[{method}] E = {out.energy:.10f} (golden {want:.10f}, d {out.energy - want:.1e}) E_D {ex['E_D']:.10f} (golden {t['E_D']:.10f})")
        assert abs(out.energy - want) < 1e-8 and abs(ex["E_D"] - t["E_D"]) < 1e-8 and ex["E_D"] == ex["E_direct"] + ex["E_indirect"]
        assert abs(ex["E_transition"] - (t["omega"] + t["E_D"])) < 1e-8 and str(ex["state_types"][0]) == "triplet"
        text = "\n".join(log) + "\n"
        start = text.rindex("\n ~~~~", 0, text.index("          Perturbative Doubles Correction"))
        end = text.index("\n Excitation energy is the energy difference")
        got, ref = text[start:end].split("\n"), t["text"].split("\n")
        assert len(got) == len(ref)
        for a, r in zip(got, ref):
            if "energy" in a and ":" in a:                      # the three numbers: within the input-line tolerance, the same layout
                assert a.split(":")[0] == r.split(":")[0] and len(a) == len(r) and abs(float(a.split(":")[1]) - float(r.split(":")[1])) < 2e-8, (a, r)
            else:
                assert a == r, (a, r)
        assert f" Excitation energy from {method + ':':<11} {ex['E_transition']:15.10f}" in text
    with pytest.raises(TunaError, match="needs an excited-state method"):
        energy.run("SPE : C O 1.128 : HF 6-31G : (D)", engine=engine)
    with pytest.raises(TunaError, match="doubles correction"):
        energy.run("SPE : C O 1.128 : CIS(D) 6-31G", engine=engine)
