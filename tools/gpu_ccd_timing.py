#!/usr/bin/env python3
"""LCCD and CCD at synth-400 (the bench workload: N = 400, o = 18, v = 382) with its converged RHF orbitals, warm, in one process:
tf_mp3_rhf (the yardstick: its ladder and rest stages are the work of one LCCD step), then --reps runs each of five fixed steps of LCCD
and of CCD (seconds per step = (ladder + rest) / steps: the MO blocks are made once per run), then --reps converged CCD runs at
conv_delta_E 1e-9 and AMPCONV 1e-8.  Prints one JSON line.  The per-kernel split comes from a kernel trace of this run (rocprofv3
--kernel-trace --stats).  Usage: python tools/gpu_ccd_timing.py [--reps 3] [--steps 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tuna_amd import molecule as mol  # noqa: E402
from tuna_amd.engine import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    counts = mol.synthetic_counts(400)
    atoms = mol.make_atoms(["AR", "AR"], 7.1)
    shells = mol.build_shells(atoms, {18: mol.even_tempered_basis(*counts)})
    aos = mol.expand_cartesian_aos(shells)
    nocc = 18
    with Engine(0) as eng:
        eng.set_basis(aos).build_eri(True)
        N = eng.N
        xyz, chg = [x.origin for x in atoms], [float(x.charge) for x in atoms]
        S, T, V, _, _ = eng.one_electron(xyz, chg, [0, 0, 0.5 * atoms[-1].origin[2]])
        X, _, _ = eng.orthogonaliser(S)
        _, C0 = eng.diagonalise(T + V, X)
        P0 = 2.0 * C0[:, :nocc] @ C0[:, :nocc].T
        nao = [sum(s.n_sph for s in shells if s.atom == k) for k in range(len(atoms))]
        r = eng.scf_rhf(S, T, V, 0.5 * (P0 + P0.T), float(np.sum(P0 * (T + V))), nocc, mol.nuclear_repulsion(atoms), X=X, conv="tight",
                        damping="dynamic", n_atom_ao=nao, max_iter=200)
        C, eps = r["C"], r["epsilons"]
        eng.mp3_rhf(C, eps, nocc)                                     # warm-up: rocBLAS kernels, the transformation's work pool
        mp3 = [eng.mp3_rhf(C, eps, nocc)["seconds"] for _ in range(a.reps)]
        res = {"N": N, "o": nocc, "v": N - nocc, "mp3_seconds": mp3, "mp3_ladder_plus_rest": [s[2] + s[3] for s in mp3]}
        for method in ("LCCD", "CCD"):
            eng.ccd_rhf(C, eps, nocc, method=method, max_iter=2, allow_unconverged=True)      # warm-up of this method's GEMM shapes
            runs = [eng.ccd_rhf(C, eps, nocc, method=method, max_iter=a.steps, conv_delta_E=0.0, conv_amplitudes=0.0, allow_unconverged=True)
                    for _ in range(a.reps)]
            res[method] = {"steps": a.steps, "seconds": [x["seconds"] for x in runs],
                           "seconds_per_step": [(x["seconds"][2] + x["seconds"][3]) / a.steps for x in runs],
                           "ladder_per_step": [x["seconds"][2] / a.steps for x in runs]}
        full = [eng.ccd_rhf(C, eps, nocc, method="CCD", conv_delta_E=1e-9, conv_amplitudes=1e-8) for _ in range(a.reps)]
        res["CCD_converged"] = {"n_iter": [x["n_iter"] for x in full], "wall": [x["seconds"][0] for x in full], "seconds": [x["seconds"] for x in full],
                                "E_corr": full[0]["E_corr"], "E_MP2": full[0]["E_MP2"]}
        print(json.dumps(res))


if __name__ == "__main__":
    main()
