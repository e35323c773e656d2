"""CPU: the host side of MP4(SDQ) / MP4(DQ) -- the routing of the four accepted method names up to the engine call, the refusals with
their messages, the log lines of the MP4 step against a stand-in engine, and the ctypes image of tf_mp4_rhf's arguments."""
import ctypes
import re
import types

import numpy as np
import pytest

from tuna_amd import _lib, energy
from tuna_amd._lib import TunaError
from test_host_ccd import routed


def test_parse_input_takes_the_mp4_lines():
    assert energy.parse_input("SPE : N N 1.0977 : MP4(SDQ) CC-PVTZ")[1:3] == ("MP4(SDQ)", "CC-PVTZ")
    assert energy.parse_input("spe : ne : mp4[dq] cc-pvdz : extreme")[1:4:2] == ("MP4[DQ]", ["NE"])


@pytest.mark.parametrize("name, level", [("MP4(SDQ)", "SDQ"), ("MP4[SDQ]", "SDQ"), ("MP4(DQ)", "DQ"), ("MP4[DQ]", "DQ")])
def test_run_routes_the_four_names(monkeypatch, name, level):
    c = routed(f"SPE : N N 1.0977 : {name} CC-PVTZ : TIGHT", monkeypatch)
    assert c.mp4 == level and c.method == "MP2" and c.reference == "RHF"
    assert not c.mp3 and not c.spin_component_scaling and c.coupled_cluster is None
    for keywords, match in (("ML 3", "closed-shell restricted reference"), ("DIPOLE", "finite-field"), ("POLAR", "finite-field"),
                            ("HYPER", "finite-field")):
        with pytest.raises(TunaError, match=match):
            routed(f"SPE : O O 1.2075 : {name} STO-3G : {keywords}", monkeypatch)
    with pytest.raises(TunaError, match=r"Unrestricted MP4.* closed-shell restricted reference"):
        routed(f"SPE : N N 1.0977 : U{name} STO-3G", monkeypatch)


def test_other_lines_do_not_ask_for_mp4(monkeypatch):
    for method in ("HF", "MP2", "SCS-MP2", "MP3", "SCS-MP3", "CCD", "LCCD", "B3LYP"):
        assert routed(f"SPE : N N 1.0977 : {method} STO-3G", monkeypatch).mp4 is None


@pytest.mark.parametrize("name", ["MP4", "MP4[SDTQ]", "MP4(SDTQ)"])
def test_full_mp4_is_refused_with_a_pointer_to_sdq(monkeypatch, name):
    with pytest.raises(TunaError) as e:
        routed(f"SPE : N N 1.0977 : {name} STO-3G", monkeypatch)
    assert "triples" in str(e.value) and "MP4(SDQ)" in str(e.value) and name in str(e.value)
    for other in ("MP5", "MP4(SD)", "MP4(T)", "SCS-MP4(SDQ)"):
        with pytest.raises(TunaError, match="is not supported"):
            routed(f"SPE : N N 1.0977 : {other} STO-3G", monkeypatch)


class StandInEngine:
    def __init__(self):
        self.calls = []

    def mp4_rhf(self, C, eps, n_occ, n_frozen=0, level="SDQ"):
        self.calls.append((n_occ, n_frozen, level))
        E_S = -0.004 if level == "SDQ" else 0.0
        return {"E_OS": -0.25, "E_SS": -0.0625, "E_MP2": -0.3125, "E_pp": 0.03, "E_hh": 0.01, "E_ring": -0.035, "E_MP3": 0.005,
                "E_S": E_S, "E_D": -0.012, "E_Q": 0.01, "E_MP4": E_S + -0.012 + 0.01, "seconds": [0.0] * 4}


@pytest.mark.parametrize("level", ["SDQ", "DQ"])
def test_mp4_step_of_the_energy_driver(level):
    calc = energy.Calculation(method="MP2", mp4=level)
    out = types.SimpleNamespace(molecular_orbitals=np.eye(3), epsilons=np.arange(3.0), energy=-100.0, timings={})
    eng, log = StandInEngine(), []
    energy.run_restricted_mp4(calc, types.SimpleNamespace(n_doubly_occ=2), out, eng, silent=False, log=log.append)
    assert eng.calls == [(2, 0, level)]
    E4 = (-0.004 if level == "SDQ" else 0.0) + -0.012 + 0.01
    assert out.energy == -100.0 + (-0.3125 + 0.005 + E4)
    assert (out.correlation_energy_mp2, out.correlation_energy_mp3, out.correlation_energy_mp4) == (-0.3125, 0.005, E4)
    assert out.mp4["E_D"] == -0.012 and out.mp3["E_MP3_scaled"] == 0.005 and out.mp2["E_MP2"] == -0.3125 and f"MP4({level}) energy" in out.timings
    # the reference's lines, character for character (tuna_mp.py:904-906, :1472, :1577, :1667-1682; tuna_kernel.py:1247-1262)
    want = ["\n  Same spin contribution:             -0.0625000000", "  Opposite spin contribution:         -0.2500000000",
            "\n  MP2 correlation energy:             -0.3125000000", "\n  MP3 correlation energy:              0.0050000000",
            "                      MP4 Energy  ",
            "  Triples are not included in MP4(SDQ).\n" if level == "SDQ" else "  Singles and triples are not included in MP4(DQ).\n",
            "  Singles correlation energy:         " + ("-0.0040000000" if level == "SDQ" else " 0.0000000000"),
            "  Doubles correlation energy:         -0.0120000000", "  Triples correlation energy:          0.0000000000",
            "  Quadruples correlation energy:       0.0100000000", f"\n  MP4 correlation energy:             {E4:13.10f}",
            "\n Correlation energy from MP2:         -0.3125000000", " Correlation energy from MP3:          0.0050000000",
            (" Correlation energy from MP4(SDQ): " if level == "SDQ" else " Correlation energy from MP4(DQ):  ") + f"{E4:16.10f}\n",
            " Total correlation energy:         " + f"{-0.3125 + 0.005 + E4:16.10f}\n"]
    assert log == want
    # silent: the same numbers, no text
    out2 = types.SimpleNamespace(molecular_orbitals=np.eye(3), epsilons=np.arange(3.0), energy=-100.0, timings={})
    energy.run_restricted_mp4(calc, types.SimpleNamespace(n_doubly_occ=2), out2, StandInEngine(), silent=True, log=log.append)
    assert out2.energy == out.energy and len(log) == len(want)


def test_argument_images_match_the_header():
    """tf_mp4_rhf as include/tunafock.h declares it: ten arguments, the level first after the context, then those of tf_mp3_rhf with
    e_mp4[3] before seconds"""
    import os
    assert "tf_mp4_rhf" in _lib.EXPORTS
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "tunafock.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    proto = re.search(r"int\s+tf_mp4_rhf\s*\(([^)]*)\)", hdr).group(1)
    args = [" ".join(a.split()) for a in proto.split(",")]
    assert args == ["tf_ctx *ctx", "int level", "int n_occ", "int n_frozen", "const double *C", "const double *eps", "double e_mp2[2]",
                    "double e_mp3[3]", "double e_mp4[3]", "double *seconds"]
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        vp, ci, dp = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double)
        assert L.tf_mp4_rhf.restype is ci and L.tf_mp4_rhf.argtypes == [vp, ci, ci, ci, vp, vp, dp, dp, dp, dp]
        assert L.tf_mp3_rhf.argtypes == [vp, ci, ci, vp, vp, dp, dp, dp]
        assert L.tf_mp4_rhf(None, 1, 1, 0, None, None, None, None, None, None) == -1     # TF_EINVAL without a context, no GPU touched


def test_engine_refuses_an_unknown_level_before_the_library():
    from tuna_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.N = 3
    with pytest.raises(TunaError, match="level must be"):
        Engine.mp4_rhf(eng, np.eye(3), np.arange(3.0), 2, 0, level="SDTQ")
    with pytest.raises(TunaError, match="orbitals must be"):
        Engine.mp4_rhf(eng, np.eye(4), np.arange(3.0), 2, 0)
