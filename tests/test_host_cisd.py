"""CPU: the host side of CIS(D) -- the ctypes image of tf_cis_d_result against the compiled header, the export and its prototype, the
argument checks of Engine.cis_d_rhf before any library call, the keywords (D) and [D] and their routing, and the (D) step of the energy
driver on a stand-in engine that answers with the reference program's own numbers: the printed section character for character
(tests/golden/cisd_text.json), out.energy moved by E_D, and with the flag off the output of today byte for byte."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
from test_host_cis import StandInEngine, driver_objects, keywords, routed
from tuna_amd import _lib, energy
from tuna_amd._lib import TunaError


def test_struct_image_matches_the_compiled_header(tmp_path):
    """sizeof and every offset of tf_cis_d_result as a C compiler lays out include/tunafock.h (compiled as C), against the ctypes class"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tunafock.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(tf_cis_d_result), offsetof(tf_cis_d_result, e_d), offsetof(tf_cis_d_result, e_direct), offsetof(tf_cis_d_result, e_indirect), '
                   'offsetof(tf_cis_d_result, min_denominator), offsetof(tf_cis_d_result, seconds)); return 0; }\n')
    exe = tmp_path / "layout"
    cc = os.environ.get("CC", "cc")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    R = _lib.CisDResult
    assert got == [ctypes.sizeof(R), R.e_d.offset, R.e_direct.offset, R.e_indirect.offset, R.min_denominator.offset, R.seconds.offset] == [56, 0, 8, 16, 24, 32]


def test_export_and_prototype():
    assert "tf_cis_d_rhf" in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "tunafock.h")) as f:
        header = f.read()
    assert "int tf_cis_d_rhf(tf_ctx *ctx, int n_occ, int n_frozen, const double *C, const double *eps, int n_states," in header
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        assert L.tf_cis_d_rhf.restype is ctypes.c_int and len(L.tf_cis_d_rhf.argtypes) == 10
        assert L.tf_cis_d_rhf.argtypes[-1] is ctypes.POINTER(_lib.CisDResult)
        assert L.tf_cis_d_rhf(None, 1, 0, None, None, 1, None, None, None, None) == -1          # TF_EINVAL without a context


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) although an argument is wrong")


def test_engine_method_checks_its_arguments_before_the_library():
    from tuna_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.N, eng._L, eng._ctx = 6, NoLibrary(), None
    C, eps, b = np.eye(6), np.arange(6.0), np.zeros((2, 2, 4))
    good = dict(b=b, omega=[0.3, 0.4], triplet=[0, 1])
    for args, kw, why in (((np.eye(5), eps, 2), good, "orbitals must be"), ((C, np.zeros(5), 2), good, "orbitals must be"),
                          ((C, eps, 2, 2), good, "windows"), ((C, eps, 6), good, "windows"), ((C, eps, 2, -1), good, "windows"),
                          ((C, eps, 2), dict(good, b=np.zeros((2, 2, 3))), r"b must be \[n_states, 2, 4\]"),
                          ((C, eps, 2), dict(good, b=np.zeros((0, 2, 4)), omega=[], triplet=[]), "n_states >= 1"),
                          ((C, eps, 2), dict(good, b=np.zeros(8)), "b must be"),
                          ((C, eps, 3, 1), dict(good, b=np.zeros((2, 2, 4))), r"b must be \[n_states, 2, 3\]"),
                          ((C, eps, 2), dict(good, omega=[0.3]), "one entry per state"), ((C, eps, 2), dict(good, triplet=[0]), "one entry per state"),
                          ((C, eps, 2), dict(good, triplet=[0, 2]), "0 .singlet. or 1 .triplet."), ((C, eps, 2), dict(good, triplet=[0.5, 1]), "0 .singlet. or 1"),
                          ((C, eps, 2), dict(b=b[0], omega=[0.3, 0.4], triplet=[0, 1]), "one entry per state")):
        with pytest.raises(TunaError, match=why):
            Engine.cis_d_rhf(eng, *args, **kw)
    with pytest.raises(TypeError):
        Engine.cis_d_rhf(eng, C, eps, 2, 0, b, [0.3, 0.4], [0, 1])           # b, omega and triplet are keyword-only

    class Recorder:                                                           # a good call reaches the library with what the header says
        def tf_cis_d_rhf(self, ctx, n_occ, n_frozen, pC, pe, n, pb, pw, pf, res):
            self.seen = (n_occ, n_frozen, n)
            r = res._obj
            for k, p in enumerate((r.e_d, r.e_direct, r.e_indirect, r.min_denominator)):
                ctypes.cast(p, ctypes.POINTER(ctypes.c_double))[0] = k + 1.0
            r.seconds[1] = 7.0
            return 0
    eng._L, eng._check = Recorder(), lambda rc: None
    r = Engine.cis_d_rhf(eng, C, eps, 2, b=b[0], omega=0.3, triplet=True)    # one state without the leading axis
    assert eng._L.seen == (2, 0, 1) and [r[k][0] for k in ("E_D", "E_direct", "E_indirect", "min_denominator")] == [1.0, 2.0, 3.0, 4.0]
    assert r["seconds"] == [0.0, 7.0, 0.0] and r["E_D"].shape == (1,)


def test_keywords_and_routing(monkeypatch):
    assert not keywords("").do_perturbative_doubles and not energy.Calculation().do_perturbative_doubles
    assert keywords("(D)").do_perturbative_doubles and keywords("[D] NSTATES 4").do_perturbative_doubles
    for line, name in (("SPE : C O 1.128 : CIS 6-31G : (D)", "CIS"), ("SPE : C O 1.128 : CIS 6-31G : [d] ROOT 2", "CIS"),
                       ("SPE : C O 1.128 : TDHF 6-31G : (D)", "TDHF"), ("SPE : C O 1.128 : RPA 6-31G : [D]", "RPA"),
                       ("SPE : C O 1.128 : HF 6-31G : TD (D)", "TD-HF"), ("SPE : C O 1.128 : RHF 6-31G : (D) TD", "TD-HF")):
        c = routed(line, monkeypatch)
        assert c.do_perturbative_doubles and c.excited_state == name, line
    for line in ("SPE : C O 1.128 : CIS 6-31G", "SPE : C O 1.128 : TDHF 6-31G : NSTATES 5", "SPE : C O 1.128 : HF 6-31G : TD"):
        assert not routed(line, monkeypatch).do_perturbative_doubles
    for line in ("SPE : C O 1.128 : HF 6-31G : (D)", "SPE : C O 1.128 : MP2 6-31G : [D]", "SPE : C O 1.128 : CCD 6-31G : (D)",
                 "SPE : C O 1.128 : B3LYP 6-31G : (D)", "SPE : C O 1.128 : HF 6-31G : TDA (D)"):
        with pytest.raises(TunaError, match="needs an excited-state method"):
            routed(line, monkeypatch)
    # the method names stay refused, now with a pointer to the keyword
    for name in ("CIS(D)", "CIS[D]", "UCIS(D)", "UCIS[D]"):
        with pytest.raises(TunaError, match="doubles correction") as e:
            routed(f"SPE : C O 1.128 : {name} 6-31G", monkeypatch)
        assert "keyword (D)" in str(e.value)


@pytest.fixture(scope="module")
def cases(golden):
    z, zd = golden("cis_systems"), golden("cisd_systems")
    with open(os.path.join(GOLD, "cis_text.json")) as f:
        cis_texts = {t["method"]: t for t in json.load(f)}
    with open(os.path.join(GOLD, "cisd_text.json")) as f:
        texts = json.load(f)
    out = []
    for t in texts:
        g = {k.split("__", 1)[1]: z[k] for k in z.files if k.startswith(t["system"] + "__")}
        d = {k.split("__", 1)[1]: zd[k] for k in zd.files if k.startswith(t["system"] + "__")}
        out.append((t, cis_texts[t["method"]], g, d))
    return out


class StandInWithDoubles(StandInEngine):
    """StandInEngine that also answers cis_d_rhf: the golden E_D of the state whose b it is handed, split arbitrarily but exactly"""

    def __init__(self, g, d, pre, vec, n_states):
        super().__init__(g, pre, vec, n_states)
        self.d, self.doubles = d, []

    def cis_d_rhf(self, C, eps, n_occ, n_frozen=0, *, b, omega, triplet):
        self.doubles.append((n_occ, n_frozen, np.array(b), list(omega), list(triplet)))
        n = int(np.argmin([np.abs(np.array(b)[0] - x).max() for x in self.d[self.pre + "b"]]))
        assert np.abs(np.array(b)[0] - self.d[self.pre + "b"][n]).max() < 1e-12 and abs(omega[0] - self.d[self.pre + "omega"][n]) < 1e-12
        E_D = float(self.d[self.pre + "E_D"][n])
        return {"E_D": np.array([E_D]), "E_direct": np.array([E_D - 0.25]), "E_indirect": np.array([0.25]),
                "min_denominator": np.array([float(self.d[self.pre + "min_denominator"][n])]), "seconds": [0.0] * 3}


def test_the_section_is_the_reference_s_and_the_energy_moves_by_E_D(cases):
    assert [t["method"] for t, _, _, _ in cases] == ["CIS", "TDHF"]
    for t, tc, g, d in cases:
        logs, outs, engines = {}, {}, {}
        for flag in (False, True):
            calc = keywords(f"NSTATES {tc['n_states']}" + (" (D)" if flag else ""))
            calc.excited_state, calc.tamm_dancoff_approximation = t["method"], t["method"] == "CIS"
            molecule, integrals, out = driver_objects(g, calc)
            eng, log = StandInWithDoubles(g, d, t["prefix"], tc["vectors"], tc["n_states"]), []
            energy.run_excited_states(calc, molecule, integrals, out, eng, silent=False, log=log.append)
            logs[flag], outs[flag], engines[flag] = "\n".join(log) + "\n", out, eng
        # the flag off: no call, and the output of the step as it was (test_host_cis pins it against the reference's)
        assert not engines[False].doubles and "E_D" not in outs[False].excited and "Doubles" not in logs[False]
        E0, E_D = float(g[t["prefix"] + "energies"][0]), t["E_D"]
        assert outs[False].energy == float(g["E_SCF"]) + E0 and E0 == t["omega"] and float(g["E_SCF"]) == t["E_SCF"]
        # the flag on: one call with the root's X + Y, its energy and its label
        (n_occ, n_frozen, b, omega, triplet), = engines[True].doubles
        X, Y = g[tc["vectors"] + "X"][0], g[tc["vectors"] + "Y"][0]
        assert (n_occ, n_frozen) == (int(g["n_occ"]), 0) and b.shape == (1,) + X.shape and np.array_equal(b[0], X + Y)
        assert omega == [E0] and triplet == [t["triplet"]] == [int(g[t["prefix"] + "labels"][0])]
        ex = outs[True].excited
        assert ex["E_D"] == E_D and ex["E_direct"] == E_D - 0.25 and ex["E_indirect"] == 0.25 and ex["E_transition"] == E0 + E_D
        assert outs[True].energy == float(g["E_SCF"]) + E0 + E_D
        assert {k: v for k, v in ex.items() if k in outs[False].excited and k != "E_transition"}.keys() == (outs[False].excited.keys() - {"E_transition"})
        # the text: today's up to the end of the spectrum, then the reference's section character for character, then the summary lines
        # with the corrected energy
        end = logs[False].index("\n Excitation energy is the energy difference")
        assert logs[True][:end] == logs[False][:end]
        rest = logs[True][end:]
        assert rest.startswith(t["text"]), (rest, t["text"])
        assert rest[len(t["text"]):] == (f"\n Excitation energy is the energy difference to excited state 1.\n\n Excitation energy from "
                                         f"{t['method'] + ':':<11} {E0 + E_D:15.10f}\n")
        # silent: the same numbers, nothing printed
        calc = keywords("(D)")
        calc.excited_state, calc.tamm_dancoff_approximation = t["method"], t["method"] == "CIS"
        molecule, integrals, out = driver_objects(g, calc)
        quiet = []
        energy.run_excited_states(calc, molecule, integrals, out, StandInWithDoubles(g, d, t["prefix"], tc["vectors"], tc["n_states"]), silent=True,
                                  log=quiet.append)
        assert not quiet and out.energy == outs[True].energy


def test_the_flag_off_is_byte_identical_on_every_keyword_of_the_step(cases):
    """NOTRIPLETS, ROOT, NSTATES and EXTHRESH with and without an unrelated spelling of the line: without (D) nothing of the step changes,
    and the stand-in is never asked for a correction"""
    t, tc, g, d = cases[0]
    for text in ("", "ROOT 3", "NSTATES 12 EXTHRESH 5", "NOTRIPLETS ROOT 2"):
        calc = keywords(text)
        assert not calc.do_perturbative_doubles
        calc.excited_state, calc.tamm_dancoff_approximation = "CIS", True
        molecule, integrals, out = driver_objects(g, calc)
        eng, log = StandInWithDoubles(g, d, t["prefix"], tc["vectors"], tc["n_states"]), []
        energy.run_excited_states(calc, molecule, integrals, out, eng, silent=False, log=log.append)
        assert not eng.doubles and "Perturbative" not in "\n".join(log) and set(out.excited) == {
            "energies", "state_types", "transition_dipoles", "oscillator_strengths", "X", "Y", "E_transition", "root", "method", "seconds", "E_singlet",
            "E_triplet", "tdm_singlet"}
