"""CPU: the work-space plan of the excited-state and stability drivers (tuna_amd/csrc/tf_excited_plan.h, compiled with g++ through
tests/excited_plan_model).  For the restricted, the unrestricted and the two stability drivers, over shapes with dim = 1, o = 1, v = 1,
an empty spin block, o_alpha != o_beta, n_keep = 0, dim and more, CIS and TDHF and every choice of multiplicities: the sections of the
small array lie in the documented order, none overlaps another, each has the length its consumer reads, the total is the closed formula
the drivers used to spell out, and the work space of the TDHF reduction is dim^2 + 3 max(1, nk) dim.  The header includes no HIP."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "tuna_amd", "csrc", "tf_excited_plan.h")
_LIB = None
SECTIONS = ("w", "w2", "e", "stat", "eps", "D_ia", "mu", "f", "C_o", "C_v", "DC_v", "D")      # the documented order
SCALARS = ("total", "square", "n_square", "kept_rows", "tdhf", "message", "tda")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(HERE, "excited_plan_model", "_build", "libexcitedplan.so")
        src = [os.path.join(HERE, "excited_plan_model", "excited_plan.cpp"), HEADER]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
            subprocess.check_call(["sh", os.path.join(HERE, "excited_plan_model", "build.sh")])
        L = C.CDLL(so)
        L.excm_rhf.argtypes = [C.c_int] * 7 + [C.c_void_p]
        L.excm_uhf.argtypes = [C.c_int] * 6 + [C.c_void_p]
        L.excm_stability.argtypes = [C.c_int] * 3 + [C.c_void_p]
        assert L.excm_sections() == len(SECTIONS)
        _LIB = L
    return _LIB


def plan(fn, *args):
    out = np.zeros(len(SECTIONS) + 1 + len(SCALARS), dtype=np.int64)
    getattr(lib(), fn)(*args, out.ctypes.data)
    p = dict(zip(SCALARS, (int(x) for x in out[len(SECTIONS) + 1:])))
    p["off"] = [int(x) for x in out[:len(SECTIONS) + 1]]
    return p


def check_sections(p, lengths):
    """in the documented order, one after the other without gap or overlap, each as long as its consumer reads, and nothing after the last"""
    off = p["off"]
    assert off[0] == 0 and off[-1] == p["total"]
    for k, name in enumerate(SECTIONS):
        assert off[k + 1] - off[k] == lengths[name], name
    spans = [(off[k], off[k + 1]) for k in range(len(SECTIONS)) if off[k + 1] > off[k]]
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


def solve_lengths(N, dim, spins, o, v):
    # w, w2: eigenvalues; e: dsyevd's off-diagonal work; stat: the two numbers of tdhf_roots_kernel; eps per spin; D_ia and mu three
    # components per element / state; f per state; C_o, C_v as uploaded; D C_v the GEMM's result; D the three dipole matrices
    return {"w": dim, "w2": dim, "e": dim, "stat": 2, "eps": spins * N, "D_ia": 3 * dim, "mu": 3 * dim, "f": dim, "C_o": N * o, "C_v": N * v,
            "DC_v": N * v, "D": 3 * N * N}


def keeps(dim):
    return [0, 1, dim, dim + 3]                                # the caller clamps: nk = min(n_keep, dim)


RHF_SHAPES = [(2, 1, 1), (5, 1, 4), (5, 4, 1), (6, 1, 1), (7, 2, 5), (10, 3, 6), (40, 7, 33)]      # N, o, v (o + v <= N: a frozen core)
MULTS = [(1, 0), (0, 1), (1, 1)]


@pytest.mark.parametrize("N,o,v", RHF_SHAPES)
def test_restricted_driver(N, o, v):
    dim = o * v
    for tda, (sing, trip), n_keep in itertools.product((0, 1), MULTS, keeps(dim)):
        nk = min(n_keep, dim)
        p = plan("excm_rhf", N, o, v, tda, sing, trip, nk)
        check_sections(p, solve_lengths(N, dim, 1, o, v))
        assert p["total"] == 3 * dim + 2 + N + 7 * dim + N * o + 2 * N * v + 3 * N * N
        assert p["square"] == dim * dim and p["kept_rows"] == max(1, nk) * dim and p["tda"] == tda
        assert p["tdhf"] == dim * dim + 3 * max(1, nk) * dim
        n_mats = sing + trip + (0 if tda else 2)
        assert p["n_square"] == n_mats + 1                      # the matrices and the transposed (ij|ab)
        assert p["message"] == (n_mats + 1) * dim * dim + (0 if tda else 3 * max(1, nk) * dim) + p["total"]


# N, (o, v) of alpha, (o, v) of beta: dim = 1 with an empty beta block (o_beta = 0); v_beta = 0; o_alpha != o_beta; equal blocks
UHF_SHAPES = [(2, (1, 1), (0, 2)), (3, (2, 1), (3, 0)), (4, (1, 3), (0, 4)), (6, (3, 3), (2, 4)), (6, (1, 5), (1, 5)), (9, (4, 5), (2, 7)),
              (40, (8, 32), (6, 34))]


@pytest.mark.parametrize("N,a,b", UHF_SHAPES)
def test_unrestricted_driver(N, a, b):
    d = [a[0] * a[1], b[0] * b[1]]
    dim, omax, vmax = d[0] + d[1], max(a[0], b[0]), max(a[1], b[1])
    assert dim >= 1
    for tda, n_keep in itertools.product((0, 1), keeps(dim)):
        nk = min(n_keep, dim)
        p = plan("excm_uhf", N, dim, omax, vmax, tda, nk)
        lengths = solve_lengths(N, dim, 2, omax, vmax)
        check_sections(p, lengths)
        for (o, v), ds in zip((a, b), d):                       # the one pair of buffers holds either spin that has excitations
            assert ds == 0 or (N * o <= lengths["C_o"] and N * v <= lengths["C_v"] and N * v <= lengths["DC_v"])
        assert p["total"] == 3 * dim + 2 + 2 * N + 7 * dim + N * omax + 2 * N * vmax + 3 * N * N
        assert p["square"] == dim * dim and p["tda"] == tda
        assert p["tdhf"] == dim * dim + 3 * max(1, nk) * dim
        assert p["n_square"] == (1 if tda else 2)
        assert p["message"] == p["n_square"] * dim * dim + p["total"]


@pytest.mark.parametrize("spins", [1, 2])
def test_stability_drivers(spins):
    shapes = [(N, o * v) for N, o, v in RHF_SHAPES] if spins == 1 else [(N, a[0] * a[1] + b[0] * b[1]) for N, a, b in UHF_SHAPES]
    for N, dim in shapes:
        p = plan("excm_stability", N, dim, spins)
        lengths = dict.fromkeys(SECTIONS, 0)
        lengths.update(w=dim, e=dim, eps=spins * N)             # eigenvalues, dsyevd's work, eps per spin: w | e | eps
        check_sections(p, lengths)
        assert p["total"] == (2 * dim + N if spins == 1 else 2 * dim + 2 * N)
        assert p["n_square"] == (4 if spins == 1 else 2)
        assert p["message"] == p["n_square"] * dim * dim + p["total"]


def test_large_shapes_do_not_wrap():
    """dim at the drivers' limit of 2 000 000 and N = 2000: every size in 64 bits"""
    N, o, v = 2000, 1000, 1000
    dim = o * v
    p = plan("excm_rhf", N, o, v, 0, 1, 1, dim)
    assert p["square"] == dim * dim and p["tdhf"] == dim * dim + 3 * dim * dim and p["message"] == 5 * dim * dim + 3 * dim * dim + p["total"]
    assert p["total"] == 10 * dim + 2 + N + N * o + 2 * N * v + 3 * N * N


def test_header_is_free_of_hip():
    src = open(HEADER).read()
    assert "#include <hip" not in src and "rocblas" not in src and "rocsolver" not in src and "hipDeviceProp" not in src
    assert [l for l in src.splitlines() if l.startswith("#include")] == ["#include <algorithm>", "#include <cstddef>"]
