#!/usr/bin/env python3
"""MP3 at synth-400 (the bench workload: N = 400, o = 18, v = 382) with its converged RHF orbitals: the stage times of tf_mp3_rhf on
the packed layout, and, in the same process on the same pair matrices T_ij = C_v t_ij C_v^T, the exchange-build route through
tf_fock_jk (Z_ij = K[T_ij^T], one general density per build) for --kpairs pairs, scaled to all o^2 pairs.  The ladder kernel's own time
comes from a kernel trace of this run (rocprofv3 --kernel-trace --stats).  Usage: python tools/gpu_mp3_timing.py [--reps 2] [--kpairs 32]
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
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--kpairs", type=int, default=32)
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
        runs = []
        for _ in range(a.reps):
            runs.append(eng.mp3_rhf(C, eps, nocc))
        best = min(runs, key=lambda x: x["seconds"][0])
        o, v = nocc, N - nocc
        # the exchange-build route on the same T matrices (host-made): Z_ij = K[T_ji], T_ji = T_ij^T
        Co, Cv = C[:, :nocc], C[:, nocc:]
        Cf = [np.ascontiguousarray(x) for x in (Co, Cv, Co, Cv)]
        g = np.empty((o, v, o, v))
        eng._check(eng._L.tf_ao_to_mo(eng._ctx, o, Cf[0].ctypes.data, v, Cf[1].ctypes.data, o, Cf[2].ctypes.data, v, Cf[3].ctypes.data,
                                      g.ctypes.data))
        D = eps[:o, None, None, None] - eps[None, o:, None, None] + eps[None, None, :o, None] - eps[None, None, None, o:]
        t = (g / D).transpose(0, 2, 1, 3)
        k = min(a.kpairs, o * o)
        pairs = [(p // o, p % o) for p in range(k)]
        Tji = np.stack([Cv @ t[j, i] @ Cv.T for i, j in pairs])
        eng.fock_jk(Tji[:2])                                          # warm-up
        t0 = time.perf_counter()
        eng.fock_jk(Tji)
        tk = time.perf_counter() - t0
        res = {"N": N, "o": o, "v": v, "E_MP3": best["E_MP3"], "terms": [best["E_pp"], best["E_hh"], best["E_ring"]],
               "seconds": {"wall": best["seconds"][0], "mo_blocks": best["seconds"][1], "ladder": best["seconds"][2], "rest": best["seconds"][3]},
               "all_runs_wall": [x["seconds"][0] for x in runs],
               "kbuild_route": {"pairs_timed": k, "seconds": tk, "seconds_per_pair": tk / k, "scaled_to_all_pairs": tk / k * o * o},
               "ladder_kernel_flops_executed_est": None}
        # executed FP64 matrix-core work of mp3_ladder_kernel: every stored value is read twice, each read feeds 64 pair columns
        # (4 MFMA column tiles) -> 2 * 64 * 2 flops per stored value and batch; the stored values are the tensor's nonzero slots
        st = eng.eri_storage()
        nbatch = -(-o * o // 64)
        res["ladder_kernel_flops_executed_est"] = 2.0 * 2.0 * 64 * (st["bytes"] / 8) * nbatch
        print(json.dumps(res))


if __name__ == "__main__":
    main()
