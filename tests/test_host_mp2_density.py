"""CPU: the host side of the MP2 densities -- the ctypes images of tf_mp2_density_opts and tf_mp2_density_result against the compiled
header, the exports and their prototypes, TF_EINVAL without a context, the argument checks of Engine.mp2_density_rhf and
Engine.natural_orbitals before any library call, the keywords RELAXED, UNRELAXED and NATORBS, and the refusals of the lines that carry
them but have no density."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from tuna_amd import _lib, energy
from tuna_amd._lib import TunaError


def test_struct_images_match_the_compiled_header(tmp_path):
    """sizeof and every offset of the two structs as a C compiler lays out include/tunafock.h (compiled as C), against the ctypes classes"""
    fields_o, fields_r = ("relaxed", "c_os", "c_ss"), ("e_os", "e_ss", "P_mo", "P_ao", "L", "z", "seconds")
    terms = ["sizeof(tf_mp2_density_opts)"] + [f"offsetof(tf_mp2_density_opts, {f})" for f in fields_o] + ["sizeof(tf_mp2_density_result)"] + \
            [f"offsetof(tf_mp2_density_result, {f})" for f in fields_r]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "tunafock.h"\nint main(void) { printf("' + "%zu " * len(terms) + '\\n", ' +
                   ", ".join(terms) + "); return 0; }\n")
    exe = tmp_path / "layout"
    cc = os.environ.get("CC", "cc")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    O, R = _lib.Mp2DensityOpts, _lib.Mp2DensityResult
    want = [ctypes.sizeof(O)] + [getattr(O, f).offset for f in fields_o] + [ctypes.sizeof(R)] + [getattr(R, f).offset for f in fields_r]
    assert got == want == [24, 0, 8, 16, 88, 0, 8, 16, 24, 32, 40, 48]


def test_exports_prototypes_and_header_text():
    assert "tf_mp2_density_rhf" in _lib.EXPORTS and "tf_natural_orbitals" in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "tunafock.h")) as f:
        header = f.read()
    assert "int tf_mp2_density_rhf(tf_ctx *ctx, const tf_mp2_density_opts *opts, int n_occ, int n_frozen, const double *C, const double *eps," in header
    assert "int tf_natural_orbitals(tf_ctx *ctx, int n, const double *P, const double *X, double *occ, double *orbitals);" in header
    for phrase in ("(A + B) z = -L", "No block with three virtual indices is formed", "singlet-unstable RHF solution -- is TF_ELINALG",
                   "at most 6 arrays of o^2 v^2 values at a time", "two calls return the same bits"):
        assert phrase in header, phrase
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        assert L.tf_mp2_density_rhf.restype is ctypes.c_int and len(L.tf_mp2_density_rhf.argtypes) == 7
        assert L.tf_mp2_density_rhf.argtypes[1] is ctypes.POINTER(_lib.Mp2DensityOpts)
        assert L.tf_mp2_density_rhf.argtypes[-1] is ctypes.POINTER(_lib.Mp2DensityResult)
        assert L.tf_natural_orbitals.restype is ctypes.c_int and len(L.tf_natural_orbitals.argtypes) == 6
        assert L.tf_mp2_density_rhf(None, None, 1, 0, None, None, None) == -1                    # TF_EINVAL without a context
        assert L.tf_natural_orbitals(None, 2, None, None, None, None) == -1


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) although an argument is wrong")


def test_engine_methods_check_their_arguments_before_the_library():
    from tuna_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.N, eng._L, eng._ctx = 6, NoLibrary(), None
    C, eps = np.eye(6), np.arange(6.0)
    for args, kw, why in (((np.eye(5), eps, 2), {}, "orbitals must be"), ((C, np.zeros(5), 2), {}, "orbitals must be"), ((C, eps, 2, 2), {}, "windows"),
                          ((C, eps, 6), {}, "windows"), ((C, eps, 0), {}, "windows"), ((C, eps, 2, -1), {}, "windows"),
                          ((C, eps, 3, 1), dict(relaxed=True), "n_frozen = 0")):
        with pytest.raises(TunaError, match=why):
            eng.mp2_density_rhf(*args, **kw)
    for P, X in ((np.eye(3), np.eye(4)), (np.zeros((3, 4)), np.eye(3)), (np.zeros(3), np.eye(3)), (np.zeros((0, 0)), np.zeros((0, 0)))):
        with pytest.raises(TunaError, match="square matrices of one size"):
            eng.natural_orbitals(P, X)


def test_keywords():
    calc = energy.interpret_keywords([], energy.Calculation())
    assert not (calc.relaxed_density or calc.unrelaxed_density or calc.natural_orbitals) and not energy.mp2_density_requested(calc)
    for words, want in ((["RELAXED"], (True, False, False)), (["UNRELAXED"], (False, True, False)), (["NATORBS"], (False, False, True)),
                        (["TIGHT", "RELAXED", "NATORBS"], (True, False, True))):
        calc = energy.interpret_keywords(words, energy.Calculation())
        assert (calc.relaxed_density, calc.unrelaxed_density, calc.natural_orbitals) == want and energy.mp2_density_requested(calc)
    with pytest.raises(TunaError, match="not supported on the GPU hot path"):
        energy.interpret_keywords(["RELAXD"], energy.Calculation())


@pytest.mark.parametrize("line,why", [
    ("SPE : C O 1.128 : UMP2 6-31G : ML 3 RELAXED", "unrestricted MP2 density is not built"),
    ("SPE : C O 1.128 : MP2 6-31G : ML 3 NATORBS", "unrestricted MP2 density is not built"),
    ("SPE : C O 1.128 : USCS-MP2 6-31G : ML 3 UNRELAXED", "unrestricted MP2 density is not built"),
    ("SPE : C O 1.128 : MP3 6-31G : NATORBS", "MP2 density on an MP3 line is not built"),
    ("SPE : C O 1.128 : SCS-MP3 6-31G : RELAXED", "MP2 density on an SCS-MP3 line is not built"),
    ("SPE : C O 1.128 : MP4(SDQ) 6-31G : RELAXED", r"MP2 density on an MP4\(SDQ\) line is not built"),
    ("SPE : C O 1.128 : CCD 6-31G : RELAXED", "coupled-cluster density is not built"),
    ("SPE : C O 1.128 : LCCD 6-31G : NATORBS", "coupled-cluster density is not built"),
    ("SPE : C O 1.128 : CIS 6-31G : UNRELAXED", "excited-state densities are not built"),
    ("SPE : C O 1.128 : TDHF 6-31G : NATORBS", "excited-state densities are not built"),
    ("SPE : C O 1.128 : HF 6-31G : TD RELAXED", "excited-state densities are not built"),
    ("SPE : C O 1.128 : HF 6-31G : NATORBS", "of a HF line are not built"),
    ("SPE : C O 1.128 : MP2 6-31G : RELAXED UNRELAXED", "two different MP2 densities"),
])
def test_refusals_name_what_is_not_built(line, why):
    """every refusal comes before an engine exists (no GPU here) and names the closed-shell MP2 / SCS-MP2 line that does have a density"""
    with pytest.raises(TunaError, match=why) as e:
        energy.run(line)
    assert "two different" in str(e.value) or "closed-shell restricted MP2 or SCS-MP2 line" in str(e.value)
