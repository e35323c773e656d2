#!/usr/bin/env python3
"""GPU timing of unrestricted MP2 on the bench workload (synth-400, converged RHF orbitals, 18 doubly occupied): tf_mp2_rhf against
tf_mp2_uhf with n_alpha = 19, n_beta = 17 on the same orbitals and with n_alpha = n_beta = 18, in one process, warm (min of --reps).
For the kernel table run it once more, on its own, under `rocprofv3 --kernel-trace --stats -- python tools/gpu_ump2_timing.py --reps 2`."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import bench  # noqa: E402
from tuna_amd import molecule as mol  # noqa: E402
from tuna_amd._lib import TunaError  # noqa: E402
from tuna_amd.engine import Engine  # noqa: E402


def converged_orbitals(eng, atoms, shells, aos, nocc):
    """The RHF cycle of the bench leg (core guess from tf_diagonalise, TIGHT, undamped first, dynamic damping if that fails)."""
    eng.set_basis(aos).build_eri(True)
    xyz, chg = [a.origin for a in atoms], [float(a.charge) for a in atoms]
    S, T, V, _, _ = eng.one_electron(xyz, chg, [0, 0, 0.5 * atoms[-1].origin[2]])
    X, _, _ = eng.orthogonaliser(S)
    _, C0 = eng.diagonalise(T + V, X)
    P0 = 2.0 * C0[:, :nocc] @ C0[:, :nocc].T
    P0 = 0.5 * (P0 + P0.T)
    nao = [sum(s.n_sph for s in shells if s.atom == a) for a in range(len(atoms))]
    args = (S, T, V, P0, float(np.sum(P0 * (T + V))), nocc, mol.nuclear_repulsion(atoms))
    try:
        r = eng.scf_rhf(*args, X=X, conv="tight", damping="none", n_atom_ao=nao, max_iter=100)
    except TunaError:
        r = eng.scf_rhf(*args, X=X, conv="tight", damping="dynamic", n_atom_ao=nao, max_iter=200)
    return r["C"], r["epsilons"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    atoms, shells, aos, nocc, desc = bench.build_workload("synth-400")
    with Engine(0) as eng:
        C, eps = converged_orbitals(eng, atoms, shells, aos, nocc)

        def best(f):
            f()                                                   # warm: the work space of the transformation is allocated once
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                r = f()
                ts.append(time.perf_counter() - t0)
            return min(ts), r
        t_r, rr = best(lambda: eng.mp2_rhf(C, eps, nocc))
        t_u1, ru1 = best(lambda: eng.mp2_uhf(C, C, eps, eps, nocc + 1, nocc - 1))
        t_u0, ru0 = best(lambda: eng.mp2_uhf(C, C, eps, eps, nocc, nocc))
    print(f"synth-400 N = {len(eps)}: RMP2 (o = {nocc}) {t_r * 1e3:.2f} ms, E_MP2 {rr['E_MP2']:.12f}")
    print(f"UMP2 n_alpha = {nocc + 1}, n_beta = {nocc - 1}: {t_u1 * 1e3:.2f} ms (ratio {t_u1 / t_r:.2f}), E_MP2 {ru1['E_MP2']:.12f}")
    print(f"UMP2 n_alpha = n_beta = {nocc}: {t_u0 * 1e3:.2f} ms (ratio {t_u0 / t_r:.2f}), E_MP2 {ru0['E_MP2']:.12f} "
          f"(RMP2 - UMP2 {rr['E_MP2'] - ru0['E_MP2']:.1e})")


if __name__ == "__main__":
    main()
