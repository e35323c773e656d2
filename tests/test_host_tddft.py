"""CPU: the host side of TD-DFT / TDA -- TD on the line of a local-density functional is routed to the excited-state step with the
name the reference prints ("TD-" + functional), the functional and its share of exact exchange; every keyword of an HF ... : TD line is
honoured; what stays refused is refused with its message; the excited-state step calls tddft_rhf with the SCF density and HFX_prop and
prints the reference's block (tests/golden/tddft_text.json) from a stand-in engine that answers with the reference's own states; the
ctypes image of tf_tddft_opts."""
import ctypes
import json
import os
import types

import numpy as np
import pytest

import xc_kernel_reference as xk
from conftest import GOLD
from test_host_cis import driver_objects, keywords, routed
from tuna_amd import _lib, dft, energy
from tuna_amd._lib import TunaError


def test_td_available_is_the_reference_s_list():
    """tuna_util.py:1445-1452 without HF (an HF line is TDHF) and SPW (no such functional here)"""
    assert set(dft.TD_AVAILABLE) == {"HFS", "SVWN", "LSDA", "LDA", "SVWN3", "SVWN5"}
    for name in dft.TD_AVAILABLE:
        xn, cn, dfx, hfx, dfc = dft.FUNCTIONALS[name]
        assert xn == "S" and cn in (None, "VWN5", "VWN3") and hfx == 0.0
        assert xk.FUNCTIONALS[name] == (xn, cn, dfx, hfx, dfc)
    assert "B3LYP" not in dft.TD_AVAILABLE and "BLYP" not in dft.TD_AVAILABLE


@pytest.mark.parametrize("functional", list(dft.TD_AVAILABLE))
def test_run_routes_the_td_dft_lines(monkeypatch, functional):
    c = routed(f"SPE : C O 1.128 : {functional} 6-31G : TD", monkeypatch)
    assert (c.excited_state, c.tamm_dancoff_approximation, c.functional, c.method, c.reference) == ("TD-" + functional, False, functional, functional, "RHF")
    assert c.time_dependent and not c.do_perturbative_doubles and not c.stability_analysis
    c = routed(f"SPE : C O 1.128 : {functional} 6-31G : TD TDA NSTATES 5 ROOT 2 NOSINGLETS EXTHRESH 5 LOOSEGRID", monkeypatch)
    assert (c.excited_state, c.tamm_dancoff_approximation, c.functional) == ("TD-" + functional, True, functional)
    assert (c.n_states, c.root, c.calculate_no_singlets, c.calculate_no_triplets, c.excited_state_contribution_threshold, c.grid_conv) == (5, 2, True, False, 5.0, "loose")
    c = routed(f"SPE : C O 1.128 : {functional} 6-31G : TD STATE 3 NOTRIPLETS", monkeypatch)
    assert (c.root, c.calculate_no_singlets, c.calculate_no_triplets) == (3, False, True)
    # without TD the line is the ground state it was; TDA alone asks for nothing
    for tail in ("", " : TDA"):
        assert routed(f"SPE : C O 1.128 : {functional} 6-31G{tail}", monkeypatch).excited_state is None


REFUSED = [("SPE : C O 1.128 : B3LYP 6-31G : TD", "HF or RHF line only"), ("SPE : C O 1.128 : BLYP 6-31G : TD", "HF or RHF line only"),
           ("SPE : C O 1.128 : BHLYP 6-31G : TD TDA", "HF or RHF line only"), ("SPE : C O 1.128 : SLYP 6-31G : TD", "HF or RHF line only"),
           ("SPE : C O 1.128 : B3LYP 6-31G : TD", "exchange-correlation kernel"),
           ("SPE : C O 1.128 : MP2 6-31G : TD", "HF or RHF line only"), ("SPE : C O 1.128 : CCD 6-31G : TD", "HF or RHF line only"),
           ("SPE : C O 1.128 : UHF 6-31G : TD", "HF or RHF line only"), ("SPE : O O 1.2075 : ULDA STO-3G : TD ML 3", "HF or RHF line only"),
           ("SPE : O O 1.2075 : LDA STO-3G : TD ML 3", "closed-shell restricted reference"),
           ("SPE : C O 1.128 : SVWN 6-31G : TD (D)", "perturbative doubles correction of a TD-DFT state"),
           ("SPE : C O 1.128 : LDA 6-31G : TD [D]", "perturbative doubles correction of a TD-DFT state"),
           ("SPE : C O 1.128 : LDA 6-31G : TD DIPOLE", "finite-field properties"), ("SPE : C O 1.128 : HFS 6-31G : TD POLAR", "finite-field properties"),
           ("SPE : C O 1.128 : SVWN3 6-31G : TD TDA HYPER", "finite-field properties"),
           ("SPE : C O 1.128 : LDA 6-31G : TD NOSINGLETS NOTRIPLETS", "There are no excited states to calculate!"),
           ("SPE : C O 1.128 : TDDFT 6-31G", "is not supported"), ("SPE : C O 1.128 : TDA 6-31G", "is not supported"),
           ("SPE : C O 1.128 : LDA 6-31G : STAB", "exchange-correlation kernel"), ("SPE : C O 1.128 : SVWN 6-31G : TD STAB", "exchange-correlation kernel"),
           ("SPE : C O 1.128 : B3LYP 6-31G : STAB", "exchange-correlation kernel")]


@pytest.mark.parametrize("line,why", REFUSED)
def test_refusals(monkeypatch, line, why):
    with pytest.raises(TunaError, match=why.replace("(", r"\(").replace(")", r"\)").replace("[", r"\[")):
        routed(line, monkeypatch)


# ---- the excited-state step of the energy driver on the reference's own numbers ----------------------------------------------------

@pytest.fixture(scope="module")
def cases(golden):
    z = golden("tddft_systems")
    with open(os.path.join(GOLD, "tddft_text.json")) as f:
        texts = json.load(f)
    return [(t, {k.split("__", 1)[1]: z[k] for k in z.files if k.startswith(t["system"] + "__")}) for t in texts]


class StandInEngine:
    """Answers tddft_rhf with the golden states of one run, as test_host_cis.StandInEngine answers cis_rhf; cis_rhf must not be called."""

    def __init__(self, g, pre, vec, n_states):
        self.g, self.pre, self.vec, self.n_states, self.calls = g, pre, vec, n_states, []

    def cis_rhf(self, *a, **k):
        raise AssertionError("a Kohn-Sham line must not reach cis_rhf")

    def tddft_rhf(self, C, eps, P, n_occ, n_frozen=0, **kw):
        self.calls.append((P, n_occ, n_frozen, {k: v for k, v in kw.items() if k != "dip"}, kw.get("dip")))
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
            for k, n in enumerate(n for n in range(self.n_states) if lab[n] == code):
                X[k], Y[k] = g[self.vec + "X"][n], g[self.vec + "Y"][n]
            out[f"X_{mult}"], out[f"Y_{mult}"] = X, Y
        return out


def ks_objects(g, calc):
    molecule, integrals, out = driver_objects(g, calc)
    out.P = g["P"]
    return molecule, integrals, out


def test_log_lines_are_the_reference_s(cases):
    assert [t["method"] for t, _ in cases] == ["TDDFT", "TDA"]
    for t, g in cases:
        tda = t["method"] == "TDA"
        calc = keywords(f"NSTATES {t['n_states']}" + (" TDA" if tda else ""))
        calc.functional, calc.HFX_prop, calc.excited_state = "SVWN", 0.0, "TD-SVWN"
        molecule, integrals, out = ks_objects(g, calc)
        eng, log = StandInEngine(g, t["prefix"], t["vectors"], t["n_states"]), []
        energy.run_excited_states(calc, molecule, integrals, out, eng, silent=False, log=log.append)
        P, n_occ, n_frozen, kw, dip = eng.calls[0]
        assert P is out.P and (n_occ, n_frozen) == (int(g["n_occ"]), 0) and dip is integrals.D and len(eng.calls) == 1
        assert kw == dict(method="TDA" if tda else "TDDFT", hfx=0.0, singlets=True, triplets=True, n_keep=t["n_states"])
        text = "\n".join(log) + "\n"
        start = text.index("\n Evaluating molecular orbitals on grid")
        end = text.index("\n Excitation energy is the energy difference")
        assert text[:start] == "\n Beginning excited state calculation...\n"
        assert text[start:end] == t["text"], (t["line"], text[start:end], t["text"])
        assert "Time-dependent Density Functional Theory" in text and ("  Using the Tamm-Dancoff" in text) == tda
        E0 = g[t["prefix"] + "energies"][0]
        assert text[end:] == (f"\n Excitation energy is the energy difference to excited state 1.\n\n Excitation energy from "
                              f"{'TD-SVWN:':<11} {E0:15.10f}\n")
        assert out.energy == float(g["E_SCF"]) + E0 and out.excited["E_transition"] == E0 and out.excited["method"] == "TD-SVWN"
        assert np.array_equal(out.excited["energies"], g[t["prefix"] + "energies"])
        assert np.array_equal(out.excited["oscillator_strengths"], g[t["prefix"] + "osc"])
        quiet = []
        molecule, integrals, out2 = ks_objects(g, calc)
        energy.run_excited_states(calc, molecule, integrals, out2, StandInEngine(g, t["prefix"], t["vectors"], t["n_states"]), silent=True, log=quiet.append)
        assert not quiet and out2.energy == out.energy


def test_hfx_prop_and_multiplicities_reach_the_engine(cases):
    t, g = cases[0]
    for text, hfx, sing, trip in (("NOTRIPLETS", 0.0, True, False), ("NOSINGLETS ROOT 2", 0.25, False, True)):
        calc = keywords(text)
        calc.functional, calc.HFX_prop, calc.excited_state = "LDA", hfx, "TD-LDA"
        molecule, integrals, out = ks_objects(g, calc)
        eng = StandInEngine(g, t["prefix"], t["vectors"], t["n_states"])
        energy.run_excited_states(calc, molecule, integrals, out, eng)
        kw = eng.calls[0][3]
        assert (kw["hfx"], kw["singlets"], kw["triplets"], kw["method"], kw["n_keep"]) == (hfx, sing, trip, "TDDFT", max(10, calc.root))
        assert set(out.excited["state_types"]) == ({"singlet"} if sing else {"triplet"})


def test_the_step_refuses_what_has_no_kernel(cases):
    t, g = cases[0]
    eng = StandInEngine(g, t["prefix"], t["vectors"], t["n_states"])
    for functional, reference, doubles, why in (("B3LYP", "RHF", False, "not yet available for this exchange-correlation functional"),
                                               ("BLYP", "RHF", False, "not yet available for this exchange-correlation functional"),
                                               ("LDA", "UHF", False, "Unrestricted time-dependent DFT is not built"),
                                               ("LDA", "RHF", True, r"The \(D\) correction of a TD-DFT state is not built")):
        calc = keywords("")
        calc.functional, calc.excited_state, calc.reference, calc.do_perturbative_doubles = functional, "TD-" + functional, reference, doubles
        molecule, integrals, out = ks_objects(g, calc)
        with pytest.raises(TunaError, match=why):
            energy.run_excited_states(calc, molecule, integrals, out, eng)
    assert not eng.calls
    calc = keywords("STAB")
    calc.functional = "LDA"
    with pytest.raises(TunaError, match="exchange-correlation kernel"):
        energy.run_stability_analysis(calc, types.SimpleNamespace(), types.SimpleNamespace(), eng)


def test_struct_image_and_exports():
    """tf_tddft_opts as include/tunafock.h lays it out (LP64): the four ints of tf_cis_opts, then hfx"""
    T = _lib.TddftOpts
    assert ctypes.sizeof(T) == 24 and (T.tda.offset, T.singlets.offset, T.triplets.offset, T.n_keep.offset, T.hfx.offset) == (0, 4, 8, 12, 16)
    assert [n for n, _ in T._fields_][:4] == [n for n, _ in _lib.CisOpts._fields_]
    for name in ("tf_xc_kernel_plan", "tf_xc_kernel_probe", "tf_xc_kernel_rhf", "tf_xc_kernel_timings", "tf_tddft_rhf"):
        assert name in _lib.EXPORTS
    header = open(os.path.join(GOLD, "..", "..", "include", "tunafock.h")).read()
    for proto in ("int tf_xc_kernel_probe(tf_ctx *ctx, int n_o, int n_v, int64_t n_points,", "int tf_xc_kernel_rhf(tf_ctx *ctx, int n_occ, int n_frozen,",
                  "int tf_tddft_rhf(tf_ctx *ctx, const tf_tddft_opts *opts, int n_occ, int n_frozen,", "} tf_tddft_opts;"):
        assert proto in header


def test_engine_methods_check_their_arguments_before_the_library():
    from tuna_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.N, eng.functional = 4, None
    with pytest.raises(TunaError, match="orbitals must be"):
        Engine.tddft_rhf(eng, np.eye(3), np.zeros(3), np.eye(4), 1)
    with pytest.raises(TunaError, match="method must be"):
        Engine.tddft_rhf(eng, np.eye(4), np.zeros(4), np.eye(4), 1, method="TDHF")
    with pytest.raises(TunaError, match="density must be"):
        Engine.tddft_rhf(eng, np.eye(4), np.zeros(4), np.eye(3), 1)
    with pytest.raises(TunaError, match="dipole matrices"):
        Engine.tddft_rhf(eng, np.eye(4), np.zeros(4), np.eye(4), 1, dip=np.zeros((3, 3, 3)))
    with pytest.raises(TunaError, match="orbitals must be"):
        Engine.xc_kernel_rhf(eng, np.eye(3), np.eye(4), 1)
    with pytest.raises(TunaError, match="density must be"):
        Engine.xc_kernel_rhf(eng, np.eye(4), np.eye(3), 1)
    with pytest.raises(ValueError, match="xc_kernel_probe"):
        Engine.xc_kernel_probe(eng, np.zeros((2, 5)), np.zeros((3, 4)), np.zeros(5), np.zeros(5))
