"""CPU: the host side of CIS / TDHF -- the keywords TD, TDA, NSTATES, ROOT / STATE, NOSINGLETS, NOTRIPLETS and EXTHRESH, the routing of
every accepted input line up to the engine call (a stand-in engine that answers with the reference program's own states of CO/6-31G),
the refusals with their messages, merging, sorting and ROOT selection, the log lines against what the reference prints
(tests/golden/cis_text.json), and the ctypes image of the tf_cis_opts / tf_cis_result structs."""
import ctypes
import json
import os
import types

import numpy as np
import pytest

from conftest import GOLD
from tuna_amd import _lib, energy
from tuna_amd._lib import TunaError


def keywords(text):
    return energy.interpret_keywords(text.split(), energy.Calculation())


def test_keywords_and_defaults():
    c = keywords("")
    assert (c.n_states, c.root, c.excited_state_contribution_threshold) == (10, 1, 1.0)
    assert not (c.time_dependent or c.tamm_dancoff_approximation or c.calculate_no_singlets or c.calculate_no_triplets) and c.excited_state is None
    c = keywords("TD TDA NSTATES 5 ROOT 3 NOTRIPLETS EXTHRESH 2.5 TIGHT")
    assert c.time_dependent and c.tamm_dancoff_approximation and c.calculate_no_triplets and not c.calculate_no_singlets
    assert (c.n_states, c.root, c.excited_state_contribution_threshold) == (5, 3, 2.5)
    assert keywords("STATE 4 NOSINGLETS").root == 4 and keywords("STATE 4 NOSINGLETS").calculate_no_singlets
    for text in ("NSTATES", "ROOT", "STATE", "EXTHRESH"):
        with pytest.raises(TunaError):
            keywords(text)


def routed(line, monkeypatch):
    seen = {}
    monkeypatch.setattr(energy, "calculate_energy", lambda symbols, R, calc, engine, silent, log: seen.setdefault("calc", calc))
    energy.run(line)
    return seen["calc"]


def test_run_routes_the_excited_state_lines(monkeypatch):
    for line, name, tda in (("SPE : C O 1.128 : CIS 6-31G", "CIS", True), ("SPE : C O 1.128 : TDHF 6-31G", "TDHF", False),
                            ("SPE : C O 1.128 : RPA 6-31G", "RPA", False), ("SPE : C O 1.128 : HF 6-31G : TD", "TD-HF", False),
                            ("SPE : C O 1.128 : RHF 6-31G : TD", "TD-HF", False), ("SPE : C O 1.128 : TDHF 6-31G : TDA", "TDHF", True),
                            ("SPE : C O 1.128 : RPA 6-31G : TDA", "RPA", True), ("SPE : C O 1.128 : HF 6-31G : TD TDA NOTRIPLETS", "TD-HF", True),
                            ("SPE : C O 1.128 : CIS 6-31G : TD", "CIS", True)):
        c = routed(line, monkeypatch)
        assert (c.excited_state, c.tamm_dancoff_approximation) == (name, tda), line
        assert c.method == "HF" and c.reference == "RHF" and not c.mp3 and c.coupled_cluster is None and c.functional is None
    c = routed("SPE : N N 1.0977 : TDHF CC-PVDZ : NSTATES 5 ROOT 2 EXTHRESH 5 NOSINGLETS EXTREME", monkeypatch)
    assert (c.n_states, c.root, c.excited_state_contribution_threshold, c.calculate_no_singlets, c.calculate_no_triplets) == (5, 2, 5.0, True, False)
    # lines without excited states stay what they were; TDA without TD asks for nothing
    for line in ("SPE : N N 1.0977 : HF STO-3G", "SPE : N N 1.0977 : HF STO-3G : TDA", "SPE : N N 1.0977 : MP2 STO-3G", "SPE : N N 1.0977 : CCD STO-3G"):
        assert routed(line, monkeypatch).excited_state is None


REFUSED = [("SPE : N N 1.0977 : CIS(D) STO-3G", "doubles correction"), ("SPE : N N 1.0977 : CIS[D] STO-3G", "doubles correction"),
           ("SPE : N N 1.0977 : UCIS STO-3G", "closed-shell restricted reference"), ("SPE : N N 1.0977 : UTDHF STO-3G", "closed-shell restricted reference"),
           ("SPE : O O 1.2075 : CIS STO-3G : ML 3", "closed-shell restricted reference"), ("SPE : O O 1.2075 : TDHF STO-3G : ML 3", "closed-shell restricted reference"),
           ("SPE : O O 1.2075 : RPA STO-3G : ML 3", "closed-shell restricted reference"), ("SPE : O O 1.2075 : HF STO-3G : TD ML 3", "closed-shell restricted reference"),
           ("SPE : N N 1.0977 : B3LYP STO-3G : TD", "HF or RHF line only"), ("SPE : N N 1.0977 : MP2 STO-3G : TD", "HF or RHF line only"),
           ("SPE : N N 1.0977 : CCD STO-3G : TD", "HF or RHF line only"), ("SPE : N N 1.0977 : UHF STO-3G : TD", "HF or RHF line only"),
           ("SPE : N N 1.0977 : CIS STO-3G : DIPOLE", "finite-field properties"), ("SPE : N N 1.0977 : TDHF STO-3G : POLAR", "finite-field properties"),
           ("SPE : N N 1.0977 : HF STO-3G : TD HYPER", "finite-field properties"),
           ("SPE : N N 1.0977 : CIS STO-3G : NOSINGLETS NOTRIPLETS", "There are no excited states to calculate!"),
           ("SPE : N N 1.0977 : HF STO-3G : TD NOSINGLETS NOTRIPLETS", "There are no excited states to calculate!")]


@pytest.mark.parametrize("line,why", REFUSED)
def test_refusals(monkeypatch, line, why):
    with pytest.raises(TunaError, match=why.replace("(", r"\(").replace(")", r"\)")):
        routed(line, monkeypatch)


def test_other_ci_names_stay_unsupported(monkeypatch):
    for name in ("CISD", "CID", "QCISD", "CIS(T)", "TDDFT", "TDA"):
        with pytest.raises(TunaError, match="is not supported"):
            routed(f"SPE : N N 1.0977 : {name} STO-3G", monkeypatch)


# ---- the excited-state step of the energy driver on the reference's own numbers ----------------------------------------------------

@pytest.fixture(scope="module")
def cases(golden):
    z = golden("cis_systems")
    with open(os.path.join(GOLD, "cis_text.json")) as f:
        texts = json.load(f)
    out = []
    for t in texts:
        g = {k.split("__", 1)[1]: z[k] for k in z.files if k.startswith(t["system"] + "__")}
        out.append((t, g))
    return out


class StandInEngine:
    """Answers cis_rhf with the golden states of one run: all energies, |mu| along z and f of the singlets in their own order, and
    the vectors of the lowest merged states handed back to their multiplicities."""

    def __init__(self, g, pre, vec, n_states):
        self.g, self.pre, self.vec, self.n_states, self.calls = g, pre, vec, n_states, []

    def cis_rhf(self, C, eps, n_occ, n_frozen=0, **kw):
        self.calls.append((n_occ, n_frozen, {k: v for k, v in kw.items() if k != "dip"}, kw.get("dip")))
        g, pre = self.g, self.pre
        lab, dim = g[pre + "labels"], len(g[pre + "E_singlet"])
        o, v = n_occ - n_frozen, len(eps) - n_occ
        out = {"dim": dim, "seconds": [0.0] * 4, "E_singlet": g[pre + "E_singlet"] if kw["singlets"] else None,
               "E_triplet": g[pre + "E_triplet"] if kw["triplets"] else None, "tdm": None, "osc": None}
        if kw["singlets"]:
            out["tdm"] = np.zeros((dim, 3))
            out["tdm"][:, 2] = g[pre + "tdm"][lab == 0]
            out["osc"] = g[pre + "osc"][lab == 0]
        nk = min(kw["n_keep"], dim)
        for code, mult in ((0, "singlet"), (1, "triplet")):
            X, Y = np.zeros((nk, o, v)), np.zeros((nk, o, v))
            mine = [n for n in range(self.n_states) if lab[n] == code]
            for k, n in enumerate(mine):
                X[k], Y[k] = g[self.vec + "X"][n], g[self.vec + "Y"][n]
            out[f"X_{mult}"], out[f"Y_{mult}"] = X, Y
        return out


def driver_objects(g, calc):
    N, nocc = len(g["eps"]), int(g["n_occ"])
    atoms = [types.SimpleNamespace(symbol="C", origin=np.zeros(3)), types.SimpleNamespace(symbol="O", origin=np.array([0.0, 0.0, 1.128 / 0.5291772105]))]
    molecule = types.SimpleNamespace(n_doubly_occ=nocc, n_basis=N, atoms=atoms)
    out = types.SimpleNamespace(molecular_orbitals=g["C"], epsilons=g["eps"], energy=float(g["E_SCF"]), timings={})
    return molecule, types.SimpleNamespace(D=g["dip"]), out


def test_log_lines_are_the_reference_s(cases):
    for t, g in cases:
        calc = keywords(f"NSTATES {t['n_states']}")
        calc.excited_state, calc.tamm_dancoff_approximation = t["method"], t["method"] == "CIS"
        molecule, integrals, out = driver_objects(g, calc)
        eng, log = StandInEngine(g, t["prefix"], t["vectors"], t["n_states"]), []
        energy.run_excited_states(calc, molecule, integrals, out, eng, silent=False, log=log.append)
        n_occ, n_frozen, kw, dip = eng.calls[0]
        assert (n_occ, n_frozen) == (int(g["n_occ"]), 0) and dip is integrals.D
        assert kw == dict(method="CIS" if t["method"] == "CIS" else "TDHF", singlets=True, triplets=True, n_keep=t["n_states"])
        text = "\n".join(log) + "\n"
        start = text.index("\n ~~~~")
        end = text.index("\n Excitation energy is the energy difference")
        assert text[:start] == "\n Beginning excited state calculation...\n"
        assert text[start:end] == t["text"], (t["line"], text[start:end], t["text"])
        E0 = g[t["prefix"] + "energies"][0]
        assert text[end:] == (f"\n Excitation energy is the energy difference to excited state 1.\n\n Excitation energy from "
                                  f"{t['method'] + ':':<11} {E0:15.10f}\n")
        assert out.energy == float(g["E_SCF"]) + E0 and out.excited["E_transition"] == E0 and out.excited["root"] == 1
        assert np.array_equal(out.excited["energies"], g[t["prefix"] + "energies"])
        assert np.array_equal(out.excited["state_types"] == "triplet", g[t["prefix"] + "labels"] == 1)
        assert np.array_equal(out.excited["transition_dipoles"], g[t["prefix"] + "tdm"])
        assert np.array_equal(out.excited["oscillator_strengths"], g[t["prefix"] + "osc"])
        assert np.array_equal(out.excited["X"], g[t["vectors"] + "X"][0]) and np.array_equal(out.excited["Y"], g[t["vectors"] + "Y"][0])
        # silent: the same numbers, nothing printed
        molecule, integrals, out2 = driver_objects(g, calc)
        quiet = []
        energy.run_excited_states(calc, molecule, integrals, out2, StandInEngine(g, t["prefix"], t["vectors"], t["n_states"]), silent=True, log=quiet.append)
        assert not quiet and out2.energy == out.energy


def test_merging_sorting_and_root_selection(cases):
    t, g = cases[0]
    pre = t["prefix"]
    e, lab = g[pre + "energies"], g[pre + "labels"]
    first_singlet = int(np.argmax(lab == 0))
    assert first_singlet > 0                                                  # CO: triplets come first
    for text, root, multiplicities in ((f"ROOT {first_singlet + 1}", first_singlet + 1, (0, 1)), ("ROOT 2 NOTRIPLETS", 2, (0,)),
                                       ("STATE 3 NOSINGLETS", 3, (1,)), ("ROOT 14 NSTATES 3", 14, (0, 1))):
        calc = keywords(text)
        calc.excited_state, calc.tamm_dancoff_approximation = "CIS", True
        molecule, integrals, out = driver_objects(g, calc)
        eng, log = StandInEngine(g, pre, t["vectors"], t["n_states"]), []
        energy.run_excited_states(calc, molecule, integrals, out, eng, silent=False, log=log.append)
        kw = eng.calls[0][2]
        assert (kw["singlets"], kw["triplets"]) == (0 in multiplicities, 1 in multiplicities) and kw["n_keep"] == max(calc.n_states, root)
        want = e[np.isin(lab, multiplicities)]
        assert np.array_equal(out.excited["energies"], want) and np.all(np.diff(out.excited["energies"]) >= 0)
        assert out.excited["E_transition"] == want[root - 1] and out.energy == float(g["E_SCF"]) + want[root - 1]
        assert set(out.excited["state_types"]) == {("singlet", "triplet")[m] for m in multiplicities}
        text_out = "\n".join(log)
        assert f"to excited state {root}." in text_out and f"{want[root - 1]:15.10f}" in text_out
        assert ("Only singlet states will be calculated." in text_out) == (multiplicities == (0,))
        assert ("Only triplet states will be calculated." in text_out) == (multiplicities == (1,))
        assert text_out.count("~~~~~ State ") == min(calc.n_states, len(want))
        if multiplicities == (0,):
            assert np.all(out.excited["oscillator_strengths"] == g[pre + "osc"][lab == 0])
    # a root beyond the states, both multiplicities off, no virtual orbitals: the reference's messages
    calc = keywords(f"ROOT {len(e) + 1}")
    calc.excited_state, calc.tamm_dancoff_approximation = "CIS", True
    molecule, integrals, out = driver_objects(g, calc)
    with pytest.raises(TunaError, match=rf"Specified root \({len(e) + 1}\) does not exist!"):
        energy.run_excited_states(calc, molecule, integrals, out, StandInEngine(g, pre, t["vectors"], t["n_states"]))
    calc = keywords("NOSINGLETS NOTRIPLETS")
    calc.excited_state = "CIS"
    with pytest.raises(TunaError, match="There are no excited states to calculate!"):
        energy.run_excited_states(calc, molecule, integrals, out, StandInEngine(g, pre, t["vectors"], t["n_states"]))
    calc = keywords("")
    calc.excited_state = "CIS"
    molecule.n_basis = molecule.n_doubly_occ
    with pytest.raises(TunaError, match="no virtual orbitals"):
        energy.run_excited_states(calc, molecule, integrals, out, StandInEngine(g, pre, t["vectors"], t["n_states"]))


def test_merge_is_the_reference_s_order():
    e, lab, src, mu, f = energy.merge_excited_states([0.3, 0.5], [0.2, 0.3, 0.6], [[0, 0, 1.0], [3.0, 4.0, 0]], [0.1, 0.2])
    assert list(e) == [0.2, 0.3, 0.3, 0.5, 0.6] and list(src) == [0, 0, 1, 1, 2]
    assert sorted(lab[1:3]) == ["singlet", "triplet"] and list(lab[[0, 3, 4]]) == ["triplet", "singlet", "triplet"]
    assert sorted(mu) == [0, 0, 0, 1.0, 5.0] and mu[3] == 5.0 and f[3] == 0.2
    e, lab, src, mu, f = energy.merge_excited_states(None, [0.4, 0.1])
    assert list(e) == [0.1, 0.4] and list(lab) == ["triplet"] * 2 and not mu.any() and not f.any()


def test_struct_images_match_the_header():
    """tf_cis_opts and tf_cis_result as include/tunafock.h lays them out (LP64)"""
    assert ctypes.sizeof(_lib.CisOpts) == 16 and _lib.CisOpts.n_keep.offset == 12 and _lib.CisOpts.singlets.offset == 4
    R = _lib.CisResult
    assert ctypes.sizeof(R) == 128 and R.dim.offset == 0 and R.e_singlet.offset == 8 and R.x_singlet.offset == 24 and R.tdm.offset == 56
    assert R.osc.offset == 64 and R.m_plus_singlet.offset == 72 and R.m_minus.offset == 88 and R.seconds.offset == 96
    assert "tf_cis_rhf" in _lib.EXPORTS


def test_engine_method_checks_its_arguments_before_the_library():
    from tuna_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.N = 4
    with pytest.raises(TunaError, match="orbitals must be"):
        Engine.cis_rhf(eng, np.eye(3), np.zeros(3), 1)
    with pytest.raises(TunaError, match="method must be"):
        Engine.cis_rhf(eng, np.eye(4), np.zeros(4), 1, method="CISD")
    with pytest.raises(TunaError, match="dipole matrices"):
        Engine.cis_rhf(eng, np.eye(4), np.zeros(4), 1, dip=np.zeros((3, 3, 3)))
