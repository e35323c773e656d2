"""GPU: LCCD and CCD of tf_ccd_rhf at the sizes where the ladder kernel's loops run more than once -- synth-200 and synth-400 -- against
the NumPy iteration from blocks (tests/ccd_reference.py: iterations_from_blocks).  No dense tensor fits, so the checker's inputs come from
quantities pinned elsewhere, as in tests/test_gpu_mp3_large.py: (ia|jb) from tf_ao_to_mo, (ij|ab) and (ik|jl) from symmetric Coulomb
matrices, Z from the general-density exchange build.  Orbitals are converged RHF orbitals (amplitudes of a few hundredths); the
synth-400 ones are those of the bench leg.  Then the full occupied window at synth-400: LCCD's first step against tf_mp3_rhf, and a
converged CCD.  Every test hands the shared context back with the default layout."""
import time

import numpy as np
import pytest

import ccd_reference as cr
import mp3_reference as mr
from test_gpu_mp2_large import _reset, _synthetic, bench_orbitals  # noqa: F401  (bench_orbitals: a fixture)
from test_gpu_mp3_large import _Z_from_exchange
from tuna_amd import molecule as mol
from tuna_amd._lib import TunaError

pytestmark = pytest.mark.gpu

METHODS = ("LCCD", "CCD")
LOOPS = {"two plain steps": (2, dict(use_diis=False), {}),
         "three steps, DIIS and damping 0.2": (3, dict(use_diis=True, damping=0.2), dict(diis=True, damping=0.2))}


def _converged_orbitals(engine, n, nocc=18):
    """RHF orbitals of the synthetic system the way the bench_orbitals fixture makes them at 400"""
    atoms, shells, aos = _synthetic(n)
    engine.set_basis(aos).build_eri(True)
    xyz, chg = [a.origin for a in atoms], [float(a.charge) for a in atoms]
    S, T, V, _, _ = engine.one_electron(xyz, chg, [0, 0, 0.5 * atoms[-1].origin[2]])
    X, _, _ = engine.orthogonaliser(S)
    _, C0 = engine.diagonalise(T + V, X)
    P0 = 2.0 * C0[:, :nocc] @ C0[:, :nocc].T
    P0 = 0.5 * (P0 + P0.T)
    nao = [sum(s.n_sph for s in shells if s.atom == a) for a in range(len(atoms))]
    args = (S, T, V, P0, float(np.sum(P0 * (T + V))), nocc, mol.nuclear_repulsion(atoms))
    try:
        r = engine.scf_rhf(*args, X=X, conv="tight", damping="none", n_atom_ao=nao, max_iter=100)
    except TunaError:
        r = engine.scf_rhf(*args, X=X, conv="tight", damping="dynamic", n_atom_ao=nao, max_iter=200)
    return aos, r["C"], r["epsilons"], nocc


def _blocks(eng, C, eps, o, nf):
    """the inputs of cr.iterations_from_blocks for the window [nf, o); no coupled-cluster or MP3 code of the library takes part"""
    Co, Cv = np.ascontiguousarray(C[:, nf:o]), np.ascontiguousarray(C[:, o:])
    ovov = eng.ao_to_mo(Co, Cv, Co, Cv)
    oovv, oooo = mr.blocks_from_coulomb(lambda D: eng.fock_jk(D)[0], Co, Cv)
    return ovov, oovv, oooo, (lambda T: _Z_from_exchange(eng, T)), Cv, eps[nf:o], eps[o:]


def _check_steps(eng, C, eps, o, nf, label):
    """max |t2 - checker| <= 1e-10 max |t| and the energy of every step to 1e-11 relative, for both methods and both loops"""
    t0 = time.perf_counter()
    blocks = _blocks(eng, C, eps, o, nf)
    bad = []
    for method in METHODS:
        for what, (k, gpu_loop, ref_loop) in LOOPS.items():
            ref = cr.iterations_from_blocks(*blocks, method, k, **ref_loop)
            r = eng.ccd_rhf(C, eps, o, nf, method=method, max_iter=k, conv_delta_E=0.0, conv_amplitudes=0.0, return_t2=True, allow_unconverged=True,
                            **gpu_loop)
            scale = np.abs(ref["t"]).max()
            dt = np.abs(r["t2"] - ref["t"]).max() / scale
            dE = np.abs(r["table"][:, 1] - np.array(ref["energies"])) / np.abs(ref["energies"])
            print(f"\n[{label} {method}, {what}] max|t| {scale:.3f} max|dt|/max|t| {dt:.1e} rel dE per step {dE} seconds {r['seconds']}")
            assert scale < 1.0 and r["n_iter"] == k
            if not (dt <= 1e-10 and np.all(dE <= 1e-11)):
                bad.append((label, method, what, dt, dE))
    print(f"[{label}] {time.perf_counter() - t0:.1f} s")
    assert not bad, bad


def test_steps_at_200(engine):
    """synth-200, o = 18: 324 pairs (five full batches of the ladder and one of 4), one block group, three column passes"""
    try:
        aos, C, eps, o = _converged_orbitals(engine, 200)
        assert engine.eri_storage()["layout"] == "packed" and engine.N == 200
        _check_steps(engine, C, eps, o, 0, "synth-200")
    finally:
        _reset(engine)


def test_steps_at_400_one_ladder_batch(engine, bench_orbitals):
    """synth-400, the occupied window cut to o = 8 by n_frozen = 10: 64 pairs, exactly one batch of the ladder, two block groups"""
    aos, C, eps, o = bench_orbitals
    try:
        engine.set_basis(aos).build_eri(True)
        assert engine.eri_storage()["layout"] == "packed" and engine.N == 400 and o == 18
        _check_steps(engine, C, eps, o, 10, "synth-400 o = 8")
    finally:
        _reset(engine)


def test_full_window_at_400(engine, bench_orbitals):
    """synth-400, o = 18: LCCD's first step is MP2 + MP3 of tf_mp3_rhf (the same contractions in another order of summation); CCD runs to
    |dE| < 1e-9 and ||dt|| < 1e-8: it converges, E_corr < E_MP2 (no reference for the value: only the sign of the difference and the
    step count are printed), t2 is symmetric under (ij)(ab), and the MO blocks are made once (their time within 1.5x of tf_mp3_rhf's)."""
    aos, C, eps, o = bench_orbitals
    try:
        engine.set_basis(aos).build_eri(True)
        assert engine.eri_storage()["layout"] == "packed" and engine.N == 400
        r3 = engine.mp3_rhf(C, eps, o)                                  # (the first call also warms rocBLAS up)
        r3 = engine.mp3_rhf(C, eps, o)
        one = engine.ccd_rhf(C, eps, o, 0, method="LCCD", max_iter=1, allow_unconverged=True)
        want = r3["E_OS"] + r3["E_SS"] + r3["E_MP3"]
        rel = abs(one["table"][0, 1] - want) / abs(want)
        print(f"\n[synth-400 o = 18] LCCD step 1 against MP2 + MP3 of mp3_rhf: rel {rel:.1e}; seconds LCCD {one['seconds']} MP3 {r3['seconds']}")
        assert rel < 1e-11
        r = engine.ccd_rhf(C, eps, o, 0, method="CCD", conv_delta_E=1e-9, conv_amplitudes=1e-8, return_t2=True)
        sym = np.abs(r["t2"] - r["t2"].transpose(1, 0, 3, 2)).max()
        print(f"[synth-400 o = 18] CCD converged {r['converged']} in {r['n_iter']} steps, sign(E_corr) {np.sign(r['E_corr']):+.0f}, "
              f"sign(E_corr - E_MP2) {np.sign(r['E_corr'] - r['E_MP2']):+.0f}, max|t2 - t2(ji,ba)| {sym:.1e}, seconds {r['seconds']}")
        assert r["converged"] and np.isfinite(r["E_corr"])
        assert sym <= 1e-14
        assert r["seconds"][1] <= 1.5 * r3["seconds"][1], (r["seconds"], r3["seconds"])
        assert r["E_corr"] < r["E_MP2"] + 0
    finally:
        _reset(engine)
