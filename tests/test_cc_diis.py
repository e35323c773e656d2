"""CPU: the host side of the coupled-cluster DIIS (tuna_amd/csrc/tf_cc_diis.h: DiisHistory and diis_solve, what tf_ccd_rhf and
tf_ccsd_rhf keep between their steps) against the DIIS part of the loop of tests/ccd_reference.iterate, step by step: which vectors
are in the history, and the extrapolation coefficients.

The model (tests/cc_diis_model) stores prescribed error vectors of length 40 the way the drivers store theirs on the device.  The
reference below is iterate's code on the same vectors: append, from step 3 on `del hist[0]` once when the history is longer than
max_diis, the bordered matrix with -1 borders through numpy.linalg.solve, and a cleared history on LinAlgError.

Tolerance: both sides are partial-pivot eliminations in double precision on matrices that agree to the rounding of their dot
products, so the coefficients agree to 64 eps cond(B) max|c|, cond(B) numpy's for the bordered matrix of that step; the vectors are
drawn so that cond(B) < 1e8, which every step checks."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LEN = 40
EPS = np.finfo(float).eps
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(HERE, "cc_diis_model", "_build", "libccdiis.so")
        src = [os.path.join(HERE, "cc_diis_model", "cc_diis_model.cpp"), os.path.join(HERE, "..", "tuna_amd", "csrc", "tf_cc_diis.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
            subprocess.check_call(["sh", os.path.join(HERE, "cc_diis_model", "build.sh")])
        L = C.CDLL(so)
        L.ccdm_random.argtypes = [C.c_uint64, C.c_int, C.c_void_p]
        L.ccdm_new.restype = C.c_void_p
        L.ccdm_new.argtypes = [C.c_int, C.c_int]
        L.ccdm_free.argtypes = [C.c_void_p]
        for f in (L.ccdm_keep, L.ccdm_nslot, L.ccdm_size):
            f.argtypes = [C.c_void_p]
        L.ccdm_step.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _LIB = L
    return _LIB


def error_vectors(case, n_steps, repeat_at=0):
    """the sequence of a case: seeded, uniform in [-1/2, 1/2); step repeat_at (if any) repeats the vector before it"""
    out = []
    for step in range(1, n_steps + 1):
        e = np.zeros(LEN)
        lib().ccdm_random(1000 * (case + 1) + step, LEN, e.ctypes.data)
        if step == repeat_at:
            e = out[-1].copy()
        out.append(e)
    return out


def run_model(max_diis, vectors):
    """per step: (slot, slots, steps, coef or None, reset, size afterwards)"""
    L = lib()
    h = L.ccdm_new(1, max_diis)
    try:
        keep, nslot = L.ccdm_keep(h), L.ccdm_nslot(h)
        rows = []
        for step, e in enumerate(vectors, 1):
            slot, solved = C.c_int(0), C.c_int(0)
            slots, steps, coef = np.zeros(33, np.int32), np.zeros(33, np.int32), np.zeros(33)
            n = L.ccdm_step(h, step, e.ctypes.data, LEN, C.byref(slot), slots.ctypes.data, steps.ctypes.data, coef.ctypes.data, C.byref(solved))
            assert 1 <= n <= nslot and 0 <= slot.value < nslot and len(set(slots[:n])) == n
            rows.append({"slot": slot.value, "slots": slots[:n].copy(), "steps": steps[:n].copy(),
                         "coef": coef[:n].copy() if solved.value == 1 else None, "reset": solved.value == -1, "size": L.ccdm_size(h)})
        return keep, nslot, rows
    finally:
        L.ccdm_free(h)


def run_reference(max_diis, vectors):
    """the DIIS part of ccd_reference.iterate on prescribed error vectors; per step: (steps in the history, coef or None, reset, B)"""
    hist_e, hist_n, rows = [], [], []
    for n, e in enumerate(vectors, 1):
        hist_e.append(e.ravel())
        hist_n.append(n)
        row = {"coef": None, "reset": False, "B": None}
        if n > 2:
            if len(hist_e) > max_diis:
                del hist_e[0], hist_n[0]
            m = len(hist_e)
            B = -np.ones((m + 1, m + 1))
            B[m, m] = 0.0
            for p in range(m):
                for q in range(m):
                    B[p, q] = float(hist_e[p] @ hist_e[q])
            rhs = np.zeros(m + 1)
            rhs[m] = -1.0
            row["B"] = B
            try:
                row["coef"] = np.linalg.solve(B, rhs)[:m]
                row["steps"] = list(hist_n)
            except np.linalg.LinAlgError:
                row["steps"] = list(hist_n)
                row["reset"] = True
                hist_e.clear()
                hist_n.clear()
        else:
            row["steps"] = list(hist_n)
        row["size"] = len(hist_e)
        rows.append(row)
    return rows


def compare(max_diis, vectors):
    """the model at max_diis against the reference at min(max_diis, 32); returns the model's rows"""
    keep, nslot, got = run_model(max_diis, vectors)
    assert keep == max(1, min(max_diis, 32)) and nslot == max(keep, 2) + 1
    want = run_reference(keep, vectors)
    for step, (g, w) in enumerate(zip(got, want), 1):
        assert list(g["steps"]) == w["steps"], (max_diis, step)
        assert g["steps"][-1] == step                       # the newest vector is the last of the history
        assert g["reset"] == w["reset"] and g["size"] == w["size"], (max_diis, step)
        assert (g["coef"] is None) == (w["coef"] is None), (max_diis, step)
        if w["coef"] is not None:
            cond = np.linalg.cond(w["B"])
            assert cond < 1e8, (max_diis, step, cond)       # the sequences are drawn to keep the systems well conditioned
            tol = 64 * EPS * cond * np.abs(w["coef"]).max()
            assert np.abs(g["coef"] - w["coef"]).max() <= tol, (max_diis, step, np.abs(g["coef"] - w["coef"]).max(), tol)
            assert abs(g["coef"].sum() - 1.0) <= tol * len(w["coef"])
    return got


N_STEPS = 70            # at max_diis = 32 the 33 slots are each written at least twice


@pytest.mark.parametrize("case,max_diis", list(enumerate([1, 2, 3, 6, 32, 40])))
def test_history_and_coefficients(case, max_diis):
    got = compare(max_diis, error_vectors(case, N_STEPS))
    keep = min(max_diis, 32)
    assert not any(g["reset"] for g in got)
    assert [len(g["steps"]) for g in got[:2]] == [1, 2]     # steps 1 and 2 store without dropping
    for step, g in enumerate(got, 1):
        assert len(g["steps"]) == min(step, max(keep, 2)), step   # (one vector leaves per step: depth 1 keeps two as well)


def test_depths_one_and_two_are_the_same_loop():
    """max_diis 1 and 2 both keep two vectors from step 3 on (one vector leaves per step): identical histories and coefficients"""
    vectors = error_vectors(0, N_STEPS)
    _, n1, one = run_model(1, vectors)
    _, n2, two = run_model(2, vectors)
    assert n1 == n2 == 3
    for step, (a, b) in enumerate(zip(one, two), 1):
        assert list(a["steps"]) == list(b["steps"]) and list(a["slots"]) == list(b["slots"]), step
        if step > 2:
            assert len(a["steps"]) == 2 and np.array_equal(a["coef"], b["coef"]), step


def test_every_slot_is_reused():
    _, nslot, got = run_model(32, error_vectors(4, N_STEPS))
    assert nslot == 33
    writes = np.bincount([g["slot"] for g in got], minlength=nslot)
    assert writes.min() >= 2, writes
    for step, g in enumerate(got, 1):
        assert list(g["steps"]) == list(range(max(1, step - 31), step + 1))


def test_repeated_vector_resets_the_history():
    """step 9 repeats the error vector of step 8: two equal rows make the bordered matrix exactly singular, both sides clear their
    history, and storing resumes with the next step (one vector, coefficient 1)"""
    got = compare(6, error_vectors(6, N_STEPS, repeat_at=9))
    assert [step for step, g in enumerate(got, 1) if g["reset"]] == [9]
    assert got[8]["size"] == 0 and got[8]["coef"] is None
    assert list(got[9]["steps"]) == [10] and got[9]["coef"][0] == 1.0
    assert list(got[10]["steps"]) == [10, 11]
    assert list(got[20]["steps"]) == list(range(16, 22))


def test_without_diis_there_are_no_slots():
    L = lib()
    h = L.ccdm_new(0, 6)
    try:
        assert L.ccdm_nslot(h) == 0 and L.ccdm_size(h) == 0
    finally:
        L.ccdm_free(h)
