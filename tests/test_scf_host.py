"""CPU: the host arithmetic of an SCF iteration (tuna_amd/csrc/tf_scf_host.h: DiisHistory with small_solve, damping_factor_tail,
scf_converged -- what run_rhf and run_uhf keep between their device stages) against the reference's bookkeeping restated in NumPy.

History.  The model (tests/scf_host_model) stores prescribed error vectors the way the cycles store theirs on the device.  The
reference below is the loop of oracle/scf_oracle.run_rhf on the same vectors: append, `del hist[0]` when the list is longer than
max_diis, the bordered matrix with -1 borders through numpy.linalg.solve, a cleared history on LinAlgError.  Every step solves.
The vectors have length 40, except at depth 64: more than 40 vectors of length 40 are linearly dependent, their bordered matrix is
singular and no bound on its condition number can hold, so that depth draws vectors of length 400.

Tolerance (as tests/test_cc_diis.py derives it): both sides are partial-pivot eliminations in double precision on matrices that agree
to the rounding of their dot products, so the coefficients agree to 64 eps cond(B) max|c|, cond(B) numpy's for the bordered matrix of
that step; the vectors are drawn so that cond(B) < 1e8, which every step checks.

Damping tail and convergence test: the same expressions as oracle/scf_oracle.py (its lines after the four _mulliken calls, and its
return condition), in the same order, on IEEE doubles: exact equality."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(float).eps
DEPTHS = [1, 2, 3, 6, 8, 64]
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(HERE, "scf_host_model", "_build", "libscfhost.so")
        src = [os.path.join(HERE, "scf_host_model", "scf_host_model.cpp"), os.path.join(HERE, "..", "tuna_amd", "csrc", "tf_scf_host.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
            subprocess.check_call(["sh", os.path.join(HERE, "scf_host_model", "build.sh")])
        L = C.CDLL(so)
        L.shm_random.argtypes = [C.c_uint64, C.c_int, C.c_void_p]
        L.shm_new.restype = C.c_void_p
        L.shm_new.argtypes = [C.c_int]
        L.shm_free.argtypes = [C.c_void_p]
        L.shm_size.argtypes = [C.c_void_p]
        L.shm_step.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.shm_damping.restype = C.c_double
        L.shm_damping.argtypes = [C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.shm_converged.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double]
        _LIB = L
    return _LIB


def length(depth):
    return 400 if depth > 32 else 40


def n_steps(depth):
    return 3 * depth + 20                # every physical slot is written at least three times


def error_vectors(case, depth, repeat_at=0):
    """the sequence of a case: seeded, uniform in [-1/2, 1/2); step repeat_at (if any) repeats the vector before it"""
    out = []
    for step in range(1, n_steps(depth) + 1):
        e = np.zeros(length(depth))
        lib().shm_random(1000 * (case + 1) + step, len(e), e.ctypes.data)
        if step == repeat_at:
            e = out[-1].copy()
        out.append(e)
    return out


def run_model(depth, vectors):
    L = lib()
    h = L.shm_new(depth)
    try:
        rows = []
        for step, e in enumerate(vectors, 1):
            slot, solved = C.c_int(0), C.c_int(0)
            slots, steps, coef = np.zeros(depth, np.int32), np.zeros(depth, np.int32), np.zeros(depth)
            n = L.shm_step(h, step, e.ctypes.data, len(e), C.byref(slot), slots.ctypes.data, steps.ctypes.data, coef.ctypes.data, C.byref(solved))
            assert 1 <= n <= depth and 0 <= slot.value < depth
            assert len(set(slots[:n])) == n and slots[n - 1] == slot.value          # each physical slot once; the newest is the last
            rows.append({"slot": slot.value, "steps": list(steps[:n]), "coef": coef[:n].copy() if solved.value == 1 else None,
                         "reset": solved.value == -1, "size": L.shm_size(h)})
        return rows
    finally:
        L.shm_free(h)


def run_reference(depth, vectors):
    """the DIIS bookkeeping of oracle/scf_oracle.run_rhf on prescribed error vectors, solving at every step"""
    hist_e, hist_n, rows = [], [], []
    for step, e in enumerate(vectors, 1):
        hist_e.append(e)
        hist_n.append(step)
        if len(hist_e) > depth:
            del hist_e[0], hist_n[0]
        n = len(hist_e)
        errs = np.array(hist_e)
        B = np.empty((n + 1, n + 1))
        B[:n, :n] = errs @ errs.T
        B[:n, -1] = -1
        B[-1, :n] = -1
        B[-1, -1] = 0
        rhs = np.zeros(n + 1)
        rhs[-1] = -1
        row = {"steps": list(hist_n), "B": B, "coef": None, "reset": False}
        try:
            row["coef"] = np.linalg.solve(B, rhs)[:n]
        except np.linalg.LinAlgError:
            row["reset"] = True
            hist_e.clear()
            hist_n.clear()
        row["size"] = len(hist_e)
        rows.append(row)
    return rows


def compare(depth, vectors):
    got, want = run_model(depth, vectors), run_reference(depth, vectors)
    for step, (g, w) in enumerate(zip(got, want), 1):
        assert g["steps"] == w["steps"], (depth, step)                       # which entries are held, oldest first
        assert g["reset"] == w["reset"] and g["size"] == w["size"], (depth, step)
        if w["reset"]:
            assert g["coef"] is None
            continue
        cond = np.linalg.cond(w["B"])
        assert cond < 1e8, (depth, step, cond)                               # the sequences are drawn to keep the systems well conditioned
        tol = 64 * EPS * cond * np.abs(w["coef"]).max()
        assert np.abs(g["coef"] - w["coef"]).max() <= tol, (depth, step, np.abs(g["coef"] - w["coef"]).max(), tol)
        assert abs(g["coef"].sum() - 1.0) <= tol * len(w["coef"])
    return got


@pytest.mark.parametrize("case,depth", list(enumerate(DEPTHS)))
def test_history_and_coefficients(case, depth):
    got = compare(depth, error_vectors(case, depth))
    assert not any(g["reset"] for g in got)
    for step, g in enumerate(got, 1):
        assert g["steps"] == list(range(max(1, step - depth + 1), step + 1)), step
    writes = np.bincount([g["slot"] for g in got], minlength=depth)
    assert writes.min() >= 3, writes                                         # every physical slot reused at least twice


def test_repeated_vector_resets_the_history():
    """step 9 repeats the error vector of step 8: two equal rows make the bordered matrix exactly singular, both sides clear their
    history, and the next step starts a new one (one vector, coefficient 1) in the slot the permutation then names"""
    got = compare(6, error_vectors(6, 6, repeat_at=9))
    assert [step for step, g in enumerate(got, 1) if g["reset"]] == [9]
    assert got[8]["size"] == 0 and got[8]["coef"] is None
    assert got[9]["steps"] == [10] and abs(got[9]["coef"][0] - 1.0) <= 4 * EPS
    assert got[10]["steps"] == [10, 11]
    assert got[20]["steps"] == list(range(16, 22))


def oracle_factor(A_n_out, A_n1_in, A_n1_out, A_n2_in, partition_ranges, max_damping):
    """oracle/scf_oracle.run_rhf, the lines after its four _mulliken calls (populations as _mulliken returns them: two entries)"""
    A_n_out, A_n1_in, A_n1_out, A_n2_in = (np.array(x, float) for x in (A_n_out, A_n1_in, A_n1_out, A_n2_in))
    den = A_n_out - A_n1_out - A_n1_in + A_n2_in
    alpha = (A_n_out - A_n1_out) / den if den.all() != 0 else [0, 0]
    if len(partition_ranges) == 2:
        factor = (alpha[0] * partition_ranges[0] + alpha[1] * partition_ranges[1]) / (partition_ranges[0] + partition_ranges[1])
    else:
        factor = alpha[0] * partition_ranges[0]
    factor = max(factor, 0)
    return float(factor if factor < min(max_damping, 1) else max_damping)


DAMPING_CASES = {   # name: (A_n_out, A_n1_in, A_n1_out, A_n2_in, partition_ranges, max_damping)
    "one partition (second population zero, as _mulliken returns it)": ([6.9, 0.0], [7.3, 0.0], [0.2, 0.0], [0.1, 0.0], [10], 0.7),
    "one partition, both denominators non-zero": ([0.31, 0.2], [0.01, 0.1], [0.3, 0.05], [0.1, 0.02], [3], 0.7),
    "two partitions": ([3.4, 3.7], [0.7, 0.9], [0.3, 0.1], [7.6, 6.3], [5, 3], 0.7),
    "two partitions, unrestricted form (zero matrices)": ([3.4, 3.7], [3.9, 3.3], [0.0, 0.0], [0.0, 0.0], [5, 5], 0.7),
    "zero denominator": ([3.4, 3.7], [3.1, 3.7], [0.3, 0.0], [0.7, 0.0], [5, 3], 0.7),
    "negative result": ([3.4, 3.7], [4.6, 4.9], [0.3, 0.1], [0.2, 0.4], [5, 3], 0.7),
    "above max_damping": ([3.4, 3.7], [3.3, 3.5], [0.3, 0.1], [0.7, 0.9], [5, 3], 0.7),
    "max_damping above 1, result below 1": ([3.4, 3.7], [0.2, 0.2], [0.3, 0.1], [0.7, 0.9], [5, 3], 1.5),
    "max_damping above 1, result above 1": ([3.4, 3.7], [3.3, 3.5], [0.3, 0.1], [0.7, 0.9], [5, 3], 1.5),
}


@pytest.mark.parametrize("name", list(DAMPING_CASES))
def test_damping_tail_is_the_oracles(name):
    """the caller's part as run_rhf forms it (pop0 - pop2 over pop0 - pop2 - pop1 + pop3), the tail from tf_scf_host.h"""
    out, in1, out1, in2, ranges, max_damping = DAMPING_CASES[name]
    want = oracle_factor(out, in1, out1, in2, ranges, max_damping)
    num = np.array([out[a] - out1[a] for a in range(2)])
    den = np.array([out[a] - out1[a] - in1[a] + in2[a] for a in range(2)])
    got = lib().shm_damping(max_damping, len(ranges), ranges[0], ranges[1] if len(ranges) > 1 else 0, num.ctypes.data, den.ctypes.data)
    assert got == want, (name, got, want)
    expect = {"zero denominator": 0.0, "negative result": 0.0, "above max_damping": 0.7, "max_damping above 1, result above 1": 1.5,
              "one partition (second population zero, as _mulliken returns it)": 0.0,
              "two partitions, unrestricted form (zero matrices)": 0.7}
    if name in expect:
        assert got == expect[name], (name, got)                              # the case is the one its name says
    else:
        assert 0.0 < got < min(max_damping, 1.0), (name, got)


def test_convergence_predicate_at_every_threshold():
    """oracle/scf_oracle.run_rhf's return condition: each of the four quantities just inside and just outside its limit, either sign"""
    thr = np.array([1e-6, 1e-5, 1e-6, 1e-4])
    inside = thr * 0.5

    def conv(v):
        return lib().shm_converged(thr.ctypes.data, float(v[0]), float(v[1]), float(v[2]), float(v[3]))

    assert conv(inside) == 1 and conv(-inside) == 1
    for q in range(4):
        for sign in (1.0, -1.0):
            v = inside.copy()
            v[q] = sign * np.nextafter(thr[q], 0.0)
            assert conv(v) == 1, (q, sign)                                   # just inside
            v[q] = sign * thr[q]
            assert conv(v) == 0, (q, sign)                                   # the limit itself is outside (strict <)
            v[q] = sign * np.nextafter(thr[q], 1.0)
            assert conv(v) == 0, (q, sign)
    assert conv(np.array([np.nan, 0.0, 0.0, 0.0])) == 0
