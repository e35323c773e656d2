#!/usr/bin/env python3
"""CIS and TDHF stage seconds (tf_cis_rhf: wall, MO blocks, assembly, solves) for one system, warm, in one process, all states of both
multiplicities with the transition moments: N2/cc-pVTZ (dim 371), Ar2/cc-pVQZ (dim 1800), the synthetic diatomic at N = 200 (dim 3276)
and at N = 400 (dim 6876: three dense solves of that size; run it on its own under a generous time limit).  The orbitals are the
converged RHF orbitals of the system.  Prints one JSON line per system.
Usage: python tools/gpu_cis_timing.py [--system n2_ccpvtz|ar2_ccpvqz|synth200|synth400 ...] [--reps 2] [--methods CIS TDHF]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tuna_amd import molecule as mol  # noqa: E402
from tuna_amd.engine import Engine  # noqa: E402


def build(name):
    if name.startswith("synth"):
        counts = mol.synthetic_counts(int(name[5:]))
        atoms = mol.make_atoms(["AR", "AR"], 7.1)
        return atoms, mol.build_shells(atoms, {18: mol.even_tempered_basis(*counts)}), 18
    sym, R, basis, nocc = {"n2_ccpvtz": (["N", "N"], 1.0977, "cc-pVTZ", 7), "ar2_ccpvqz": (["AR", "AR"], 3.76, "cc-pVQZ", 18)}[name]
    atoms = mol.make_atoms(sym, mol.angstrom_to_bohr(R))
    return atoms, mol.build_shells(atoms, basis), nocc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--system", nargs="+", default=["n2_ccpvtz", "ar2_ccpvqz", "synth200"])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--methods", nargs="+", default=["CIS", "TDHF"])
    a = ap.parse_args()
    with Engine(0) as eng:
        for name in a.system:
            atoms, shells, nocc = build(name)
            aos = mol.expand_cartesian_aos(shells)
            eng.set_basis(aos).build_eri(True)
            N = eng.N
            xyz, chg = [x.origin for x in atoms], [float(x.charge) for x in atoms]
            S, T, V, D, _ = eng.one_electron(xyz, chg, [0, 0, 0.5 * atoms[-1].origin[2]])
            X, _, _ = eng.orthogonaliser(S)
            _, C0 = eng.diagonalise(T + V, X)
            P0 = 2.0 * C0[:, :nocc] @ C0[:, :nocc].T
            nao = [sum(s.n_sph for s in shells if s.atom == k) for k in range(len(atoms))]
            r = eng.scf_rhf(S, T, V, 0.5 * (P0 + P0.T), float(np.sum(P0 * (T + V))), nocc, mol.nuclear_repulsion(atoms), X=X, conv="tight",
                            damping="dynamic", n_atom_ao=nao, max_iter=200)
            C, eps = r["C"], r["epsilons"]
            res = {"system": name, "N": N, "o": nocc, "v": N - nocc, "dim": nocc * (N - nocc), "layout": eng.eri_storage()["layout"],
                   "stages": ["wall", "MO blocks", "assembly", "solves"]}
            for method in a.methods:
                runs = []
                for _ in range(a.reps):                               # (the first run carries the one-time loads of rocSOLVER's kernels)
                    t0 = time.perf_counter()
                    try:
                        x = eng.cis_rhf(C, eps, nocc, method=method, n_keep=10, dip=D)
                        runs.append({"seconds": x["seconds"], "call": time.perf_counter() - t0, "lowest_singlet": float(x["E_singlet"][0]),
                                     "lowest_triplet": float(x["E_triplet"][0]), "sum_f": float(x["osc"].sum())})
                    except Exception as e:                            # an unstable reference, or memory
                        runs.append({"error": str(e), "call": time.perf_counter() - t0})
                        break
                res[method] = runs
                print(json.dumps({"partial": name, method: runs}), flush=True)
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
