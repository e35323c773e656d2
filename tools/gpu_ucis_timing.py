#!/usr/bin/env python3
"""Unrestricted CIS / TDHF and stability stage seconds (tf_cis_uhf, tf_stability_uhf: wall, MO blocks, assembly, solves) on the synthetic
diatomic at N = 200 and N = 400 with (o_alpha, o_beta) = (10, 8), warm, in one process: the second call of each (the first carries the
one-time loads of rocSOLVER's kernels), next to tf_cis_rhf (o = 18, both multiplicities) and tf_stability_rhf of the same build.  The
orbitals are the closed-shell RHF orbitals of the system for both spins, the virtual energies of either spin --shift Eh higher (30: the
ten-and-eight-electron determinant then has positive definite A + B and A - B; with 1 Eh dpotrf stops.  A timing input, not a state of
the molecule: the work does not depend on the values).  A call that raises is reported with its message.  Prints one JSON line per
system; quote the smallest of the repetitions.
Usage: python tools/gpu_ucis_timing.py [--n 200 400] [--reps 3] [--keep 10] [--shift 30]
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
from tuna_amd._lib import TunaError  # noqa: E402
from tuna_amd.engine import Engine  # noqa: E402


def timed(call, reps):
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        try:
            r = call()
            runs.append({"seconds": r["seconds"], "call": time.perf_counter() - t0})
        except TunaError as e:
            runs.append({"error": str(e), "call": time.perf_counter() - t0})
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[200, 400])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--keep", type=int, default=10)
    ap.add_argument("--alpha", type=int, default=10)
    ap.add_argument("--beta", type=int, default=8)
    ap.add_argument("--shift", type=float, default=30.0)
    a = ap.parse_args()
    with Engine(0) as eng:
        for n in a.n:
            atoms, shells, nocc = build(f"synth{n}")
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
            na, nb = a.alpha, a.beta
            ea, eb = eps.copy(), eps.copy()
            ea[na:] += a.shift
            eb[nb:] += a.shift
            res = {"system": f"synth{n}", "N": N, "o_alpha": na, "o_beta": nb, "dim": na * (N - na) + nb * (N - nb), "dim_restricted": nocc * (N - nocc),
                   "layout": eng.eri_storage()["layout"], "stages": ["wall", "MO blocks", "assembly", "solves"]}
            for method in ("CIS", "TDHF"):
                res[f"cis_uhf {method}"] = timed(lambda: eng.cis_uhf(C, C, ea, eb, na, nb, method=method, n_keep=a.keep, dip=D), a.reps)
                res[f"cis_rhf {method}"] = timed(lambda: eng.cis_rhf(C, eps, nocc, method=method, n_keep=a.keep, dip=D), a.reps)
            res["stability_uhf"] = timed(lambda: eng.stability_uhf(C, C, ea, eb, na, nb), a.reps)
            res["stability_rhf"] = timed(lambda: eng.stability_rhf(C, eps, nocc), a.reps)
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
