#!/usr/bin/env python3
"""CIS(D) stage seconds (tf_cis_d_rhf: state-independent blocks, dressed transformations, kernels and GEMMs) on the synthetic diatomic
at N = 400 (o = 18, v = 382) or N = 200 (`--n`), warm, in one process, for 1 state and for 10 states (the five lowest singlets and the
five lowest triplets of CIS on the converged RHF orbitals), next to `cis_rhf` of the same build.  Prints one JSON line.
Usage: python tools/gpu_cisd_timing.py [--n 400] [--reps 2]
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
    ap.add_argument("--n", type=int, default=400)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    with Engine(0) as eng:
        atoms, shells, nocc = build(f"synth{a.n}")
        eng.set_basis(mol.expand_cartesian_aos(shells)).build_eri(True)
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
        res = {"system": f"synth{a.n}", "N": N, "o": nocc, "v": N - nocc, "layout": eng.eri_storage()["layout"],
               "cis_stages": ["wall", "MO blocks", "assembly", "solves"],
               "cis_d_stages": ["state-independent blocks", "dressed transformations", "kernels and GEMMs"]}
        cis = []
        for _ in range(a.reps):                                   # (the first run carries the one-time loads of rocSOLVER's kernels)
            t0 = time.perf_counter()
            x = eng.cis_rhf(C, eps, nocc, method="CIS", n_keep=5, dip=D)
            cis.append({"seconds": x["seconds"], "call": time.perf_counter() - t0})
        res["cis_rhf"] = cis
        b = np.concatenate([x["X_singlet"], x["X_triplet"]])
        w = np.concatenate([x["E_singlet"][:5], x["E_triplet"][:5]])
        flags = np.array([0] * 5 + [1] * 5)
        for n_states, pick in ((1, [0]), (10, list(range(10)))):
            runs = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                y = eng.cis_d_rhf(C, eps, nocc, b=b[pick], omega=w[pick], triplet=flags[pick])
                runs.append({"seconds": y["seconds"], "call": time.perf_counter() - t0})
            res[f"cis_d_rhf_{n_states}"] = runs
            res[f"E_D_{n_states}"] = [float(v) for v in y["E_D"]]
            res[f"min_denominator_{n_states}"] = float(y["min_denominator"].min())
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
