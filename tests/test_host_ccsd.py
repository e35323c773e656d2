"""CPU: the host side of LCCSD / QCISD / CCSD -- the ctypes image of tf_ccsd_result against include/tunafock.h (compiled, where a C
compiler is at hand), the export list, Engine.ccsd_rhf's refusals before the library, the energy driver's step against a stand-in engine
(kwargs, log lines, the TF_ENOTCONV path, silent mode) and the dispatch of calculate_energy.  The input line keeps refusing the three
names (tests/test_host_ccd.py)."""
import ctypes
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from tuna_amd import _lib, energy
from tuna_amd._lib import TunaError
from tuna_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("e_corr", "e_mp2", "e_singles", "e_connected", "e_disconnected", "t1_norm", "n_iter", "converged", "ladder_batches", "table", "t1", "t2",
          "seconds")


def test_struct_image_matches_the_header(tmp_path):
    """tf_ccsd_result as include/tunafock.h lays it out (LP64): the field order from the header text, sizes and offsets by hand and,
    with a C compiler, from offsetof"""
    R = _lib.CcsdResult
    assert tuple(n for n, _ in R._fields_) == FIELDS
    text = open(os.path.join(ROOT, "include", "tunafock.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} tf_ccsd_result;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = tuple(re.sub(r"\[.*\]", "", d.split()[-1].lstrip("*")) for d in body.split(";") if d.strip())
    assert declared == FIELDS
    assert ctypes.sizeof(R) == 120
    want = dict(e_corr=0, e_mp2=8, e_singles=16, e_connected=24, e_disconnected=32, t1_norm=40, n_iter=48, converged=52, ladder_batches=56,
                table=64, t1=72, t2=80, seconds=88)
    assert {n: getattr(R, n).offset for n in FIELDS} == want
    assert [re.search(rf"#define TF_CCSD_{n}\s+(\d)", text).group(1) for n in ("LCCSD", "QCISD", "CCSD")] == ["0", "1", "2"]
    assert Engine.CCSD_METHODS == {"LCCSD": 0, "QCISD": 1, "CCSD": 2}
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc:
        src = tmp_path / "o.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tunafock.h"\nint main(void) { printf("%zu", sizeof(tf_ccsd_result));\n'
                       + "".join(f'printf(" %zu", offsetof(tf_ccsd_result, {n}));\n' for n in FIELDS) + "return 0; }\n")
        exe = tmp_path / "o"
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
        got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
        assert got == [120] + [want[n] for n in FIELDS]
    # tf_cc_opts is reused unchanged
    assert ctypes.sizeof(_lib.CcOpts) == 40


def test_export_list_and_header():
    assert "tf_ccsd_rhf" in _lib.EXPORTS and "tf_ccd_rhf" in _lib.EXPORTS
    text = open(os.path.join(ROOT, "include", "tunafock.h")).read()
    assert re.search(r"^int tf_ccsd_rhf\(tf_ctx \*ctx, const tf_cc_opts \*opts, int n_occ, int n_frozen,\s*const double \*C, const double \*eps, "
                     r"tf_ccsd_result \*out\);", text, flags=re.M)


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


def bare_engine(N=4):
    e = Engine.__new__(Engine)
    e.N, e._L, e._ctx = N, NoLibrary(), None
    return e


def test_engine_refuses_before_the_library():
    e = bare_engine()
    C, eps = np.eye(4), np.arange(4.0)
    for method in ("CCD", "LCCD", "CCSD(T)", "ccsd", "CEPA(0)", "CISD", None, 2):
        with pytest.raises(TunaError, match="method must be"):
            e.ccsd_rhf(C, eps, 2, method=method)
    for badC, badeps in ((np.eye(3), eps), (C, np.arange(3.0)), (np.zeros((4, 5)), eps), (C, np.zeros((4, 1)))):
        with pytest.raises(TunaError, match="orbitals must be"):
            e.ccsd_rhf(badC, badeps, 2)
    with pytest.raises(TunaError, match="method must be"):        # ccd_rhf keeps refusing the singles methods
        e.ccd_rhf(C, eps, 2, method="CCSD")


class StandInEngine:
    def __init__(self, converged=True):
        self.converged, self.calls = converged, []

    def ccsd_rhf(self, C, eps, n_occ, n_frozen=0, **kw):
        self.calls.append((n_occ, n_frozen, kw))
        table = np.array([[1, -0.30, -0.30], [2, -0.31, -0.01], [3, -0.3105, -0.0005]])
        return {"E_corr": -0.3105, "E_MP2": -0.29, "E_singles": 0.0, "E_connected": -0.3100, "E_disconnected": -0.0005, "t1_norm": 0.04,
                "T1_diagnostic": 0.01, "ladder_batches": 3, "n_iter": 3, "converged": self.converged, "table": table, "seconds": [0.0] * 4}

    def ccd_rhf(self, *a, **k):
        raise AssertionError("the doubles entry point was called")


def keywords(text):
    return energy.interpret_keywords(text.split(), energy.Calculation())


@pytest.mark.parametrize("name", ["LCCSD", "QCISD", "CCSD"])
def test_ccsd_step_of_the_energy_driver(name):
    calc = keywords("EXTREME AMPCONV 1e-9 CORRDAMP 0.25 DIIS 4 ECONV 1e-7")
    calc.coupled_cluster = name
    out = types.SimpleNamespace(molecular_orbitals=np.eye(3), epsilons=np.arange(3.0), energy=-100.0, timings={})
    molecule = types.SimpleNamespace(n_doubly_occ=2)
    eng, log = StandInEngine(), []
    energy.run_coupled_cluster_singles_doubles(calc, molecule, out, eng, silent=False, log=log.append)
    n_occ, n_frozen, kw = eng.calls[0]
    assert (n_occ, n_frozen) == (2, 0)
    assert kw == dict(method=name, max_iter=100, conv_delta_E=1e-7, conv_amplitudes=1e-9, use_diis=True, max_diis=4, damping=0.25,
                      allow_unconverged=True)
    assert out.energy == -100.0 - 0.3105 and out.correlation_energy_cc == -0.3105 and out.cc["n_iter"] == 3 and f"{name} energy" in out.timings
    text = "\n".join(log)
    for s in (f"              {name:>5} Energy and Density ", "  Energy convergence tolerance:        0.0000001000",
              "  Amplitude convergence tolerance:     0.0000000010", "\n  Guess t-amplitude MP2 energy:       -0.2900000000\n",
              "  Using damping parameter of 0.25 for convergence.", "  Using DIIS, storing 4 matrices, for convergence.",
              f"\n  Starting {name} iterations...\n", "  Step          Correlation E               DE",
              "    3           -0.3105000000         -0.0005000000",
              "\n  Singles contribution:                0.0000000000", "  Connected doubles contribution:     -0.3100000000",
              "  Disconnected doubles contribution:  -0.0005000000",
              f"\n  {name} correlation energy:  {' ' * (10 - len(name))}    -0.3105000000",
              "\n  Norm of singles amplitudes:          0.0400000000", "  Value of T1 diagnostic:              0.0100000000",
              f" Correlation energy from {name}:{' ' * (8 - len(name))}    -0.3105000000\n"):
        assert s in text, s
    # silent: nothing is logged, the outputs are set all the same
    out2 = types.SimpleNamespace(molecular_orbitals=np.eye(3), epsilons=np.arange(3.0), energy=-100.0, timings={})
    log = []
    energy.run_coupled_cluster_singles_doubles(calc, molecule, out2, StandInEngine(), silent=True, log=log.append)
    assert log == [] and out2.energy == out.energy and out2.cc["E_connected"] == -0.31
    # no DIIS and no damping: neither line; a run that does not converge raises after the table
    calc = keywords("NODIIS")
    calc.coupled_cluster = name
    log = []
    with pytest.raises(TunaError) as e:
        energy.run_coupled_cluster_singles_doubles(calc, molecule, out, StandInEngine(False), silent=False, log=log.append)
    assert e.value.code == -4 and "CORRMAXITER" in str(e.value) and name in str(e.value)
    text = "\n".join(log)
    assert "Using DIIS" not in text and "Using damping" not in text and f"Starting {name} iterations..." in text and "    3   " in text
    assert "Singles contribution" not in text


def test_calculate_energy_dispatches_by_name(monkeypatch):
    """LCCSD / QCISD / CCSD go to the new step, CCD / LCCD to the old one, nothing without a name; everything in front of the
    correlated step is a stand-in"""
    seen = []
    monkeypatch.setattr(energy, "run_coupled_cluster_singles_doubles", lambda calc, *a, **k: seen.append(("sd", calc.coupled_cluster)))
    monkeypatch.setattr(energy, "run_coupled_cluster_doubles", lambda calc, *a, **k: seen.append(("d", calc.coupled_cluster)))
    molecule = types.SimpleNamespace(atoms=[], n_doubly_occ=1)
    monkeypatch.setattr(energy, "build_molecule_and_integrals", lambda symbols, R, calc, engine: (molecule, types.SimpleNamespace(), None, None, {}))
    monkeypatch.setattr(energy.mol, "nuclear_repulsion", lambda atoms: 0.0)
    monkeypatch.setattr(energy, "run_self_consistent_field_cycle",
                        lambda *a, **k: types.SimpleNamespace(energy=-1.0, timings={}, molecular_orbitals=np.eye(2), epsilons=np.arange(2.0)))
    for name in ("LCCSD", "QCISD", "CCSD", "CCD", "LCCD", None):
        calc = keywords("")
        calc.coupled_cluster = name
        out = energy.calculate_energy(["H", "H"], 1.4, calc, engine=object(), silent=True, log=None)
        assert out.energy == -1.0
    assert seen == [("sd", "LCCSD"), ("sd", "QCISD"), ("sd", "CCSD"), ("d", "CCD"), ("d", "LCCD")]
    assert energy.CCSD_METHODS == ("LCCSD", "QCISD", "CCSD")
