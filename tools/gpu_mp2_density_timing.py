#!/usr/bin/env python3
"""MP2-density stage seconds (tf_mp2_density_rhf: wall, MO blocks, ladder, Z-vector, rest) on the synthetic diatomic at N = 200 and
N = 400 (o = 18), warm, in one process: the relaxed and the unrelaxed density, the second call of each (the first carries the one-time
loads of rocSOLVER's kernels), next to `mp2_rhf` of the same build and to `natural_orbitals` of the relaxed density.  Prints one JSON
line per system.
Usage: python tools/gpu_mp2_density_timing.py [--n 200 400] [--reps 2]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gpu_cis_timing import build  # noqa: E402
from tuna_amd import molecule as mol  # noqa: E402
from tuna_amd.engine import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[200, 400])
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    with Engine(0) as eng:
        for n in a.n:
            atoms, shells, nocc = build(f"synth{n}")
            eng.set_basis(mol.expand_cartesian_aos(shells)).build_eri(True)
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
            res = {"system": f"synth{n}", "N": N, "o": nocc, "v": N - nocc, "layout": eng.eri_storage()["layout"],
                   "stages": ["wall", "MO blocks", "ladder", "Z-vector", "rest"]}
            res["mp2_rhf"] = [eng.mp2_rhf(C, eps, nocc)["seconds"] for _ in range(a.reps)]
            for kind in ("relaxed", "unrelaxed"):
                runs = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    d = eng.mp2_density_rhf(C, eps, nocc, relaxed=kind == "relaxed")
                    runs.append({"seconds": d["seconds"], "call": time.perf_counter() - t0})
                res[kind] = runs
                if kind == "relaxed":
                    t0 = time.perf_counter()
                    occ, _ = eng.natural_orbitals(d["P_ao"], X)
                    res["natural_orbitals"] = time.perf_counter() - t0
                    res["max_z"], res["trace"], res["largest_virtual_occupation"] = float(np.abs(d["z"]).max()), float(np.trace(d["P_mo"])), float(occ[nocc])
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
