#!/usr/bin/env python3
"""LCCSD, QCISD and CCSD at synth-400 (the bench workload: N = 400, o = 18, v = 382) with its converged RHF orbitals, warm, in one
process, next to CCD of the same build: --reps runs each of --steps fixed steps per method (seconds per step = (ladder + rest) / steps:
the MO blocks are made once per run), the split of `seconds`, and the pieces CCSD adds per step timed on their own through the public
entry points: one (ov|ov) AO->MO transformation with t1-dressed coefficients (tf_ao_to_mo; its copy to the host is included), one
32-virtual slice of the dressed (vv|oo) transformation scaled to v, and one general-density J/K build.  CCSD minus QCISD per step is the
cost of the two dressed transformations and the J/K build inside the call.  Prints one JSON line.
Usage: python tools/gpu_ccsd_timing.py [--reps 3] [--steps 4]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
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
        res = {"N": N, "o": nocc, "v": N - nocc}
        fixed = dict(max_iter=a.steps, conv_delta_E=0.0, conv_amplitudes=0.0, allow_unconverged=True)
        t1 = None
        for method, call in (("CCD", eng.ccd_rhf), ("LCCSD", eng.ccsd_rhf), ("QCISD", eng.ccsd_rhf), ("CCSD", eng.ccsd_rhf)):
            call(C, eps, nocc, method=method, max_iter=2, allow_unconverged=True)             # warm-up of this method's GEMM shapes
            runs = [call(C, eps, nocc, method=method, **(dict(fixed, return_t1=True) if method != "CCD" else fixed)) for _ in range(a.reps)]
            res[method] = {"steps": a.steps, "seconds": [x["seconds"] for x in runs],
                           "seconds_per_step": [(x["seconds"][2] + x["seconds"][3]) / a.steps for x in runs],
                           "ladder_per_step": [x["seconds"][2] / a.steps for x in runs],
                           "rest_per_step": [x["seconds"][3] / a.steps for x in runs], "E": runs[0]["table"][:, 1].tolist()}
            if method == "CCSD":
                t1 = runs[0]["t1"]
                res[method]["t1_norm"] = runs[0]["t1_norm"]
        # the pieces CCSD adds per step, on their own
        Co, Cv = C[:, :nocc], C[:, nocc:]
        Lo, Xv = Co + Cv @ t1.T, Cv - Co @ t1
        pieces = {"dressed_ovov": [], "dressed_vvoo_slice32": [], "jk_general": []}
        for _ in range(a.reps + 1):
            t0 = time.perf_counter(); eng.ao_to_mo(Lo, Xv, Co, Cv); pieces["dressed_ovov"].append(time.perf_counter() - t0)
            t0 = time.perf_counter(); eng.ao_to_mo(Xv[:, :32], Cv, Lo, Co); pieces["dressed_vvoo_slice32"].append(time.perf_counter() - t0)
            t0 = time.perf_counter(); eng.fock_jk(Cv @ t1.T @ Co.T); pieces["jk_general"].append(time.perf_counter() - t0)
        res["pieces"] = {k: v[1:] for k, v in pieces.items()}
        res["pieces"]["dressed_vvoo_scaled_to_v"] = [x * (N - nocc) / 32.0 for x in pieces["dressed_vvoo_slice32"][1:]]
        print(json.dumps(res))


if __name__ == "__main__":
    main()
