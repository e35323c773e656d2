"""GPU: the MP2 one-particle density (tf_mp2_density_rhf) and the natural orbitals (tf_natural_orbitals) away from the golden systems:
random orthonormal orbitals, which have no symmetry to hide a transposed index behind; occupied widths at the edges of the ladder's batches
of 64 pairs and past one pass of the amplitude kernel's grid-stride loop; small virtual spaces; frozen windows; the rows and tiles
layouts; converged orbitals at N = 120; and the Lagrangian L, element by element.  The checker is tests/mp2_density_reference.py.

Bounds.  Every element of P_oo, P_vv and L and both energies: |device - checker| <= 1e-12 S, S the checker's sum of the magnitudes of the
terms of that element (the element-level bound of the triples and MP3 checker tests; sqrt(n) 2^-53 S at the longest sum here, n = o v^2 =
1.9e5, is 5e-14 S; the checker itself is within 1e-13 S of its own longdouble evaluation, tests/test_mp2_density_reference.py).  The
diagonal of the occupied block is compared after taking the reference determinant's 2 off again (exact), and is allowed the 2^-53 by
which the device's sum 2 + P_ii is rounded.  z: max |dz| <= [ ||1e-12 S_L||_2 + (||1e-12 S_M||_F + dim 2^-53 ||A + B||_2) ||z||_2 ] /
lambda_min(A + B), first-order perturbation of the solve with a backward-stable Cholesky (z_bound).  Exact in every case: P_mo is bitwise
symmetric, its occupied-virtual block is 0.0 (unrelaxed) or 0.5 z bit for bit (relaxed); |tr P_mo - 2 n_occ| <= 1e-12 sum of the diagonal
S; P_ao against C P_mo C^T of the device's own P_mo within 1e-12 |C| |P_mo| |C^T|.  Every test hands the context back with the default
layout.

Measured on one MI355X, the worst |d| / S over all cases of a test (z and the trace in the same unit: 1e-12 is their bound):
    widths 1 ... 16     P_oo 5.0e-15  P_vv 4.4e-15  L 1.2e-15  z 1.5e-17  E_OS 1.2e-15  E_SS 3.8e-16  trace 2.7e-14  P_ao 2.0e-16
    v = 3, 2, 1         P_oo 1.8e-15  P_vv 1.1e-15  L 1.0e-15  z 2.2e-16  E_OS 1.4e-15  E_SS 4.6e-17  trace 2.2e-13  P_ao 2.8e-16
    frozen 5, 11        P_oo 6.5e-15  P_vv 4.1e-15  E_OS 1.4e-15  E_SS 1.2e-16  trace 0  P_ao 6.2e-17
    rows, tiles         P_oo 3.3e-15  P_vv 4.5e-15  L 8.3e-16  z 2.9e-18  E_OS 1.2e-15  E_SS 2.9e-16  trace 2.7e-14  P_ao 1.3e-16
                        (no array of either layout has the bits of the packed layout, at width 7 or 12, relaxed or not)
    N = 120             P_oo 5.1e-15  P_vv 3.8e-15  z 8.7e-18  E_OS 1.5e-15  E_SS 6.6e-16  trace 0  P_ao 5.0e-16;  L 2.8e-16 of its bound
                        with the integral term (test_mid_size), 2.5e-7 S_L without it, max |dL| 2.7e-15
    natural orbitals    occupations 1.6e-13, orthonormality 9.1e-15, rebuilt P 2.4e-14 (n = 33); all 0 at n = 1
The slowest test is test_mid_size at 1.8 s, the widths take 0.2 to 1.0 s each.  Of four wrong kernels tried once each, every one
failed here: the amplitude loop stopped after its first pass (widths 12, 16, both layouts, N = 120; tests/test_gpu_mp2_density.py
passed in full), (ib|ja) read from (ia|jb), the Lagrangian without the second image of the back-transformation, and the ladder's OA
batches all written at offset 0.
"""
import numpy as np
import pytest

import mp2_density_reference as mr
from test_gpu_ccd_large import _converged_orbitals
from test_gpu_mp3 import _reset, _system
from test_mp2_density_reference import DEVICE_BOUND, FROZEN, SCS, SMALL_O, WIDTHS, small_orbitals, width_orbitals, z_bound
from tuna_amd._lib import TunaError

pytestmark = pytest.mark.gpu

TF_ELINALG = -5
TOL = 1e-10                        # natural occupations, as tests/test_gpu_mp2_density.py
WEIGHTS_7 = ((1.0, 1.0), (1.0, 0.0), (0.0, 1.0))
_cache = {}


def _tensor(tag):
    """(aos, dense AO tensor) of a system, formed once"""
    if ("E", tag) not in _cache:
        shells, aos = _system(tag)
        _cache["E", tag] = (aos, mr.dense_eri(aos, shells))
    return _cache["E", tag]


def _reference(tag, C, eps, nocc, nf, weights, key):
    """the dense checker (relaxed where the window allows it: P_oo, P_vv and the energies do not depend on that), once per case"""
    key = ("ref", tag, key, nocc, nf, weights)
    if key not in _cache:
        E = _tensor(tag)[1]
        if ("g", tag, key[2]) not in _cache:
            _cache["g", tag, key[2]] = mr.mo_integrals(E, C)
        ref = mr.mp2_density(E, C, eps, nocc, nf, nf == 0, *weights, g=_cache["g", tag, key[2]])
        for k in ("P2", "S_oo", "S_vv", "L", "z", "S_L", "S_M"):
            if ref[k] is not None:
                ref[k].setflags(write=False)
        o, v = slice(nf, nocc), slice(nocc, len(eps))
        ref["P_oo"], ref["P_vv"] = ref["P2"][o, o], ref["P2"][v, v]
        _cache[key] = ref
    return _cache[key]


def _ratio(d, S):
    """max d / S with 0 / 0 = 0 (an element that symmetry makes exactly zero on both sides) and d / 0 = inf"""
    d, S = np.asarray(d, dtype=np.float64), np.asarray(S, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(d == 0.0, 0.0, d / S)))


def _check(r, ref, C, nocc, nf, relaxed, label, delta_g=0.0):
    """one device result against the checker: the exact properties, then every bound; returns {quantity: worst |d| / S}.  delta_g: an
    error of the MO integrals themselves, which adds delta_g T_L to the bound of L (test_mid_size)"""
    N = C.shape[0]
    o, v, f = slice(nf, nocc), slice(nocc, N), slice(0, nf)
    P = r["P_mo"]
    assert np.array_equal(P, P.T), label
    assert np.array_equal(P[f, f], 2.0 * np.eye(nf)) and not P[f, nf:].any(), label             # frozen orbitals: 2.0 and exact zeros
    if relaxed:
        assert np.array_equal(P[o, v], 0.5 * r["z"]), label
    else:
        assert r["L"] is None and r["z"] is None and not P[:nocc, v].any(), label
    no = nocc - nf
    dev_oo = P[o, o] - 2.0 * np.eye(no)                                                         # exact: 1 <= P_ii <= 2
    assert np.all(np.diag(P)[:nocc] > 1.0), label                                               # the occupied diagonal carries the 2
    worst = {"P_oo": _ratio(np.maximum(np.abs(dev_oo - ref["P_oo"]) - 2.0 ** -53 * np.eye(no), 0.0), ref["S_oo"]),
             "P_vv": _ratio(np.abs(P[v, v] - ref["P_vv"]), ref["S_vv"]),
             "E_OS": abs(r["E_OS"] - ref["E_OS"]) / ref["S_E_OS"], "E_SS": abs(r["E_SS"] - ref["E_SS"]) / ref["S_E_SS"]}
    if relaxed:
        worst["L"] = _ratio(np.abs(r["L"] - ref["L"]), ref["S_L"] + (delta_g / DEVICE_BOUND) * ref["T_L"])
        worst["z"] = np.abs(r["z"] - ref["z"]).max() / z_bound(ref, DEVICE_BOUND, ref["z"].size) * DEVICE_BOUND
    worst["tr"] = abs(np.trace(P) - 2 * nocc) / (np.trace(ref["S_oo"]) + np.trace(ref["S_vv"]))
    worst["P_ao"] = _ratio(np.abs(r["P_ao"] - C @ P @ C.T), np.abs(C) @ np.abs(P) @ np.abs(C.T))
    worst = {k: float(x) for k, x in worst.items()}
    print(f"\n[{label}] worst |d| / S " + " ".join(f"{k} {x:.1e}" for k, x in worst.items()) + f" seconds {r['seconds'][0]:.3f}")
    return worst


def _failures(worst, label):
    return [(label, k, x) for k, x in worst.items() if not x <= DEVICE_BOUND]


def _both_kinds(engine, tag, C, eps, nocc, weights, key, label, bad, keep=None):
    ref = _reference(tag, C, eps, nocc, 0, weights, key)
    for relaxed in (False, True):
        r = engine.mp2_density_rhf(C, eps, nocc, 0, relaxed=relaxed, c_os=weights[0], c_ss=weights[1])
        name = f"{label} c_os {weights[0]:.3f} c_ss {weights[1]:.3f} {'relaxed' if relaxed else 'unrelaxed'}"
        bad += _failures(_check(r, ref, C, nocc, 0, relaxed, name), name)
        if keep is not None:
            keep[relaxed] = r


ARRAYS = ("E_OS", "E_SS", "P_mo", "P_ao", "L", "z")


def _same_bits(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]) for k in ARRAYS)


@pytest.mark.parametrize("width", WIDTHS)
def test_widths_on_random_orbitals(engine, width):
    """N2/cc-pVTZ (N = 60), random orthonormal orbitals, SCS weights, unrelaxed and relaxed.  o = 1: one pair, v = 59; 2: the first i != j;
    7: 49 pairs, one partial batch of the ladder, and the weights (1, 1), (1, 0) and (0, 1), which isolate the operands; 8: 64 pairs, one
    full batch; 12: 144 pairs = 2 batches + 16 and o^2 v^2 = 331,776 > 262,144 threads, so the amplitude kernel's loop makes a second pass
    for part of the grid, and a second relaxed call returns the same bits; 16: 256 pairs = 4 full batches, 495,616 elements."""
    aos, _ = _tensor("n2_ccpvtz")
    engine.set_basis(aos).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed" and engine.N == 60
    C, eps = width_orbitals(engine.N, width)
    bad, keep = [], {}
    for weights in (SCS,) + (WEIGHTS_7 if width == 7 else ()):
        _both_kinds(engine, "n2_ccpvtz", C, eps, width, weights, width, f"width {width}", bad, keep if weights == SCS else None)
    if width == 12:
        again = engine.mp2_density_rhf(C, eps, width, 0, relaxed=True, c_os=SCS[0], c_ss=SCS[1])
        assert _same_bits(keep[True], again)
    assert not bad, bad


@pytest.mark.parametrize("o", SMALL_O)
def test_small_virtual_spaces(engine, o):
    """N2/STO-3G (N = 10), random orthonormal orbitals: v = 3, 2 and 1 under o = 7, 8 and 9."""
    aos, _ = _tensor("n2_sto3g")
    engine.set_basis(aos).build_eri(True)
    C, eps = small_orbitals(engine.N, o)
    bad = []
    _both_kinds(engine, "n2_sto3g", C, eps, o, SCS, ("small", o), f"o {o} v {engine.N - o}", bad)
    assert not bad, bad


@pytest.mark.parametrize("width,nf", FROZEN)
def test_frozen_windows(engine, width, nf):
    """N2/cc-pVTZ, the random orbitals of width 12, unrelaxed, 5 and 11 frozen (o = 7 and o = 1): the window's blocks against the checker,
    every frozen orbital with exactly 2.0 on the diagonal and exact zeros in the rest of its row and column."""
    aos, _ = _tensor("n2_ccpvtz")
    engine.set_basis(aos).build_eri(True)
    C, eps = width_orbitals(engine.N, width)
    ref = _reference("n2_ccpvtz", C, eps, width, nf, SCS, width)
    r = engine.mp2_density_rhf(C, eps, width, nf, c_os=SCS[0], c_ss=SCS[1])
    label = f"width {width} frozen {nf}"
    bad = _failures(_check(r, ref, C, width, nf, False, label), label)
    assert not bad, bad


@pytest.mark.parametrize("layout", ["rows", "tiles"])
def test_other_layouts_on_random_orbitals(engine, layout):
    """Widths 7 and 12 on the rows and tiles layouts: the back-transformation has one image and the ladder goes through the exchange
    build in chunks of 2 and 8 pair matrices (49 pairs: a ragged last chunk).  The same bounds; whether the bits are those of the packed
    layout is printed, not asserted."""
    aos, _ = _tensor("n2_ccpvtz")
    bad = []
    try:
        for width in (7, 12):
            C, eps = width_orbitals(60, width)
            engine.set_basis(aos).build_eri(True, layout="packed")
            packed = {}
            _both_kinds(engine, "n2_ccpvtz", C, eps, width, SCS, width, f"packed width {width}", bad, packed)
            engine.build_eri(True, layout=layout)
            assert engine.eri_storage()["layout"] == layout
            other = {}
            _both_kinds(engine, "n2_ccpvtz", C, eps, width, SCS, width, f"{layout} width {width}", bad, other)
            print(f"[{layout} width {width}] bit-identical to packed: unrelaxed {_same_bits(packed[False], other[False])} "
                  f"relaxed {_same_bits(packed[True], other[True])}")
    finally:
        _reset(engine)
    assert not bad, bad


MID_SHIFT = 1.0


def test_mid_size(engine):
    """Synthetic N = 120, converged RHF orbitals, o = 18, v = 102, MP2 weights: 324 pairs = 5 batches + 4, 3.37M amplitude elements =
    12.9 passes of the amplitude kernel's grid, dim = 1836 = 57 tiles of 32 + 12 in the assembly of A + B.  The checker is
    mp2_density_from_blocks on the MO blocks of engine.ao_to_mo: no density code of the library takes part.
    The converged orbitals of this system are singlet-unstable: the checker finds lambda_min(A + B) = -0.103 (cond 4.3e4), so their
    Z-vector equations have no meaningful solution.  With them the unrelaxed density goes against the checker and the relaxed call must
    be refused with TF_ELINALG (dpotrf at dim 1836); the relaxed comparison then runs on the same orbitals with the virtual energies
    1 Eh higher, as the random orbitals above have them, which moves every eigenvalue of A + B up by 1 (lambda_min = 0.897) and leaves
    every shape and every path as it was.
    The bound of L has a second term here.  In this even-tempered basis the transformed integrals carry an absolute error from
    cancellation over the AO indices, which no sum of MO-basis magnitudes sees: the blocks of engine.ao_to_mo, the checker's input, break their own
    permutational symmetry, (ia|bc) = (ia|cb) and the like, by delta_g = 1.6e-13 (integrals up to 0.1), and the library's AO-direct
    terms round at the same scale.  Rows of the two 1s core orbitals have |L| around 1e-10 and S_L around 5e-9; there |dL| reaches
    1.2e-15 = 2.5e-7 S_L while max |dL| over all of L is 2.7e-15 against max S_L = 0.61.  So the bound is 1e-12 S_L + delta_g T_L,
    delta_g measured in the test as that symmetry defect and T_L = sum |dL / dg| from the checker (first-order propagation); the
    1e-12 stays, and P_oo, P_vv, z and the energies keep their plain bounds."""
    try:
        aos, C, eps, nocc = _converged_orbitals(engine, 120)
        N = engine.N
        assert N == 120 and nocc == 18
        Co, Cv = np.ascontiguousarray(C[:, :nocc]), np.ascontiguousarray(C[:, nocc:])
        blocks = [engine.ao_to_mo(*cs) for cs in ((Co, Cv, Co, Cv), (Co, Co, Cv, Cv), (Co, Co, Co, Cv), (Co, Cv, Cv, Cv))]
        shifted = eps.copy()
        shifted[nocc:] += MID_SHIFT
        bad = []
        # as converged: unrelaxed, and the refusal
        ref = mr.mp2_density_from_blocks(eps[:nocc], eps[nocc:], blocks[0], None, None, None, False, 1.0, 1.0)
        ref["P_oo"], ref["P_vv"] = ref["P2"][:nocc, :nocc], ref["P2"][nocc:, nocc:]
        bad += _failures(_check(engine.mp2_density_rhf(C, eps, nocc, 0), ref, C, nocc, 0, False, "synth-120 o 18 v 102 unrelaxed"), "synth-120 unrelaxed")
        # shifted: relaxed
        ref = mr.mp2_density_from_blocks(shifted[:nocc], shifted[nocc:], *blocks, True, 1.0, 1.0)
        ref["P_oo"], ref["P_vv"] = ref["P2"][:nocc, :nocc], ref["P2"][nocc:, nocc:]
        lam0 = ref["lambda_min"] - MID_SHIFT
        print(f"\n[synth-120] lambda_min as converged {lam0:.3f}, shifted {ref['lambda_min']:.3f} cond {ref['cond']:.1f} max |z| {np.abs(ref['z']).max():.2e} "
              f"z bound {z_bound(ref, DEVICE_BOUND, ref['z'].size):.1e}")
        assert ref["D_max"] < 0 and ref["lambda_min"] > 0.5 and abs(lam0) > 1e-3
        try:
            engine.mp2_density_rhf(C, eps, nocc, 0, relaxed=True)
            refused = False
        except TunaError as e:
            assert e.code == TF_ELINALG and "not positive definite" in str(e)
            refused = True
        assert refused == (lam0 < 0)
        r = engine.mp2_density_rhf(C, shifted, nocc, 0, relaxed=True)
        ovov, oovv, ooov, ovvv = blocks
        delta_g = max(np.abs(ovvv - ovvv.transpose(0, 1, 3, 2)).max(), np.abs(ooov - ooov.transpose(1, 0, 2, 3)).max(),
                      np.abs(oovv - oovv.transpose(1, 0, 2, 3)).max(), np.abs(oovv - oovv.transpose(0, 1, 3, 2)).max(),
                      np.abs(ovov - ovov.transpose(2, 3, 0, 1)).max())
        plain = _ratio(np.abs(r["L"] - ref["L"]), ref["S_L"])
        print(f"[synth-120] delta_g {delta_g:.1e}; L against 1e-12 S_L alone: worst |d| / S {plain:.1e}, max |dL| {np.abs(r['L'] - ref['L']).max():.1e}, "
              f"max delta_g T_L {delta_g * ref['T_L'].max():.1e}")
        assert delta_g < 1e-12
        bad += _failures(_check(r, ref, C, nocc, 0, True, "synth-120 o 18 v 102 shifted relaxed", delta_g), "synth-120 relaxed")
        assert not bad, bad
    finally:
        _reset(engine)


def _orthogonaliser(n, seed):
    """(S, X = S^-1/2) of a random symmetric positive definite S with eigenvalues log-uniform in [0.1, 10] (cond <= 100)"""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    lam = 10.0 ** rng.uniform(-1.0, 1.0, n)
    return (Q * lam) @ Q.T, (Q / np.sqrt(lam)) @ Q.T


@pytest.mark.parametrize("n", [1, 2, 33])
def test_natural_orbitals_off_the_goldens(engine, n):
    """n = 1, 2 and 33 (no basis set has them): a random symmetric P and the fully degenerate P = 2 X X^T, with X = S^-1/2 of a random
    positive definite S.  Occupations within 1e-10 of the checker's and descending, the orbitals S-orthonormal and rebuilding P."""
    S, X = _orthogonaliser(n, 70 + n)
    A = np.random.default_rng(170 + n).standard_normal((n, n))
    for label, P in (("random", 0.5 * (A + A.T)), ("degenerate", 2.0 * X @ X.T)):
        occ, orb = engine.natural_orbitals(P, X)
        want = mr.natural_orbitals(P, X)[0]
        d_occ = np.abs(occ - want).max()
        d_orth = np.abs(orb.T @ S @ orb - np.eye(n)).max()
        d_P = np.abs((orb * occ) @ orb.T - P).max()
        print(f"\n[n {n} {label}] d occ {d_occ:.1e} orthonormality {d_orth:.1e} rebuilt P {d_P:.1e}")
        assert d_occ < TOL and np.all(np.diff(occ) <= 0)
        assert d_orth < 1e-10 and d_P < TOL
        if label == "degenerate":
            assert np.abs(occ - 2.0).max() < TOL
