#!/usr/bin/env python3
"""MP4(SDQ) and MP4(DQ) at synth-400 (the bench workload: N = 400, o = 18, v = 382) with its converged RHF orbitals, warm, in one
process: --reps runs of tf_mp3_rhf (the yardstick: tf_mp4_rhf's ladder share is two passes of its ladder stage; their spread is the
run-to-run spread), then --reps runs each of tf_mp4_rhf at the levels SDQ and DQ, then tf_mp3_rhf again (its own time must not depend
on what ran in between).  Prints one JSON line: the seconds of every run ([wall, MO blocks, ladder, rest]), the ladder ratio
median(MP4 ladder) / (2 median(MP3 ladder)) per level, and the relative spread (max - min) / median of the MP3 ladder times.  With
--mp3-only only the MP3 runs are made (the same measurement on a build without tf_mp4_rhf).
Usage: python tools/gpu_mp4_timing.py [--reps 5] [--mp3-only]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mp3-only", action="store_true")
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
        lad3 = [s[2] for s in mp3]
        res = {"N": N, "o": nocc, "v": N - nocc, "mp3_seconds": mp3, "mp3_wall_median": float(np.median([s[0] for s in mp3])),
               "mp3_ladder_median": float(np.median(lad3)), "mp3_ladder_spread": float((max(lad3) - min(lad3)) / np.median(lad3))}
        if not a.mp3_only:
            for level in ("SDQ", "DQ"):
                eng.mp4_rhf(C, eps, nocc, level=level)                # warm-up of this level's GEMM shapes
                runs = [eng.mp4_rhf(C, eps, nocc, level=level) for _ in range(a.reps)]
                sec = [x["seconds"] for x in runs]
                res[level] = {"seconds": sec, "wall_median": float(np.median([s[0] for s in sec])),
                              "ladder_median": float(np.median([s[2] for s in sec])), "rest_median": float(np.median([s[3] for s in sec])),
                              "ladder_ratio_to_two_mp3_passes": float(np.median([s[2] for s in sec]) / (2.0 * np.median(lad3))),
                              "E_S": runs[0]["E_S"], "E_D": runs[0]["E_D"], "E_Q": runs[0]["E_Q"],
                              "bitwise_repeatable": all(x[k] == runs[0][k] for x in runs for k in ("E_S", "E_D", "E_Q", "E_MP3", "E_MP2"))}
            after = [eng.mp3_rhf(C, eps, nocc)["seconds"] for _ in range(a.reps)]
            res["mp3_seconds_after"] = after
            res["mp3_wall_median_after"] = float(np.median([s[0] for s in after]))
        print(json.dumps(res))


if __name__ == "__main__":
    main()
