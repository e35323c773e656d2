#!/usr/bin/env python3
"""The perturbative triples (tf_triples_rhf) at a synthetic size with converged RHF orbitals (default synth-400, the bench workload:
N = 400, o = 18, v = 382; --n 200 for the half size), warm, in one process: one warm-up call, then --reps calls of kind MP4 and of kind
CCSD(T) (random amplitudes: the cost does not depend on their values).  Prints one JSON line: the seconds of every call ([wall, MO blocks
incl. (ia|bc), triples loop, rest]), the medians, the loop time per unordered triple, the GEMM flop rate the loop time implies if the GEMMs
were all of it (2 o^3 v^4 nominal, 12 n_triples v^3 (v + o) executed) and the bytes the fused kernel reads per call (6 v^3 doubles per
triple) over the loop time -- a LOWER bound of the kernel's read rate, next to the HBM figures of DESIGN.md (8 TB/s spec, 6.8 TB/s read
by tools/microbench/hbm_patterns).  The library records no events inside the loop: the split of the loop between the rocBLAS kernels and
triples_energy_kernel is NOT reported here and comes from a kernel trace of the same command (DESIGN.md has it for synth-200 only):  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/gpu_triples_timing.py --n 200 --reps 1
Usage: python tools/gpu_triples_timing.py [--n 400] [--reps 3] [--frozen 0]
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
    ap.add_argument("--n", type=int, default=400)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frozen", type=int, default=0)
    a = ap.parse_args()
    atoms = mol.make_atoms(["AR", "AR"], 7.1)
    shells = mol.build_shells(atoms, {18: mol.even_tempered_basis(*mol.synthetic_counts(a.n))})
    aos = mol.expand_cartesian_aos(shells)
    nocc, nf = 18, a.frozen
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
        o, v = nocc - nf, N - nocc
        rng = np.random.default_rng(0)
        t1, t2 = 0.01 * rng.standard_normal((o, v)), 0.01 * rng.standard_normal((o, o, v, v))
        eng.triples_rhf(C, eps, nocc, nf, kind="MP4")                 # warm-up: rocBLAS kernels, the transformation's work pool
        res = {"N": N, "o": o, "v": v}
        for kind, amps in (("MP4", {}), ("CCSD(T)", dict(t1=t1, t2=t2))):
            runs = [eng.triples_rhf(C, eps, nocc, nf, kind=kind, **amps) for _ in range(a.reps)]
            sec = np.array([x["seconds"] for x in runs])
            nt = runs[0]["n_triples"]
            loop = float(np.median(sec[:, 2]))
            res[kind] = {"seconds": sec.tolist(), "wall_median": float(np.median(sec[:, 0])), "blocks_median": float(np.median(sec[:, 1])),
                         "loop_median": loop, "loop_spread": float((sec[:, 2].max() - sec[:, 2].min()) / loop), "n_triples": nt,
                         "loop_seconds_per_triple": loop / max(1, nt), "nominal_flop": 2.0 * o ** 3 * float(v) ** 4,
                         "executed_gemm_flop": 12.0 * nt * float(v) ** 3 * (v + o),
                         "gemm_tflops_if_all_of_the_loop": 12.0 * nt * float(v) ** 3 * (v + o) / loop / 1e12,
                         "kernel_bytes_read": 48.0 * nt * float(v) ** 3, "kernel_read_TBps_lower_bound": 48.0 * nt * float(v) ** 3 / loop / 1e12,
                         "E_T": runs[0]["E_T"], "identical": all(x["E_T"] == runs[0]["E_T"] for x in runs)}
        print(json.dumps(res))


if __name__ == "__main__":
    main()
