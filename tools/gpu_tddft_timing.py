#!/usr/bin/env python3
"""TD-DFT / TDA stage seconds on the synthetic diatomic (default N = 400, o = 18: dim = 6876) with LDA on the medium grid, warm (the
second call of everything), in one process:
  * the kernel build of tf_xc_kernel_rhf split into psi GEMM, density and point kernels, K kernel and slab sum (tf_xc_kernel_timings);
  * the baseline for the K kernel: the same two matrices from torch float64 matmul (rocBLAS) on MATERIALISED slabs of the transition
    density T[g][(ia)] = psi_i psi_a, on orbital values and weights of the same shapes (random: the time does not depend on them);
  * tf_tddft_rhf TDA and full TD-DFT totals by stage, next to tf_cis_rhf CIS and TDHF on the same orbitals.
The orbitals are the converged Kohn-Sham LDA orbitals of the system.  A solve the library refuses (an unstable reference) is reported
as such, not retried.  Prints one JSON line.
Usage: python tools/gpu_tddft_timing.py [--n 400] [--grid medium] [--slab 8192]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tuna_amd import dft, molecule as mol  # noqa: E402
from tuna_amd._lib import TunaError  # noqa: E402
from tuna_amd.engine import Engine  # noqa: E402


def baseline(G, o, v, slab):
    """seconds of K_S and K_T from torch matmul on materialised T slabs, second of two passes"""
    import torch
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    psi = torch.randn(G, o + v, dtype=torch.float64, device=dev, generator=gen)
    uS, uT = (torch.randn(G, dtype=torch.float64, device=dev, generator=gen) for _ in range(2))
    dim = o * v
    secs = []
    for _ in range(2):
        KS, KT = (torch.zeros(dim, dim, dtype=torch.float64, device=dev) for _ in range(2))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for g0 in range(0, G, slab):
            p = psi[g0:g0 + slab]
            T = (p[:, :o, None] * p[:, None, o:]).reshape(-1, dim)             # [slab, dim] in HBM
            KS.addmm_(T.T, T * uS[g0:g0 + slab, None])
            KT.addmm_(T.T, T * uT[g0:g0 + slab, None])
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    del psi, KS, KT
    torch.cuda.empty_cache()
    return secs[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=400)
    ap.add_argument("--grid", default="medium")
    ap.add_argument("--slab", type=int, default=8192)
    a = ap.parse_args()
    import torch                                                # (torch initialises the device first: two copies of the HIP runtime in one
    torch.cuda.set_device(0)                                    #  process otherwise, tests/test_gpu_fock_shapes.py)
    torch.zeros(1, device="cuda:0")
    nocc = 18
    atoms = mol.make_atoms(["AR", "AR"], 7.1)
    shells = mol.build_shells(atoms, {18: mol.even_tempered_basis(*mol.synthetic_counts(a.n))})
    aos = mol.expand_cartesian_aos(shells)
    with Engine(0) as eng:
        eng.set_basis(aos).build_eri(True)
        N = eng.N
        pts, wts, _ = dft.integration_grid(atoms, a.grid)
        f = eng.dft_setup(pts, wts, "LDA")
        G = f["n_points"]
        xyz, chg = [x.origin for x in atoms], [float(x.charge) for x in atoms]
        S, T, V, D, _ = eng.one_electron(xyz, chg, [0, 0, 0.5 * atoms[-1].origin[2]])
        X, _, _ = eng.orthogonaliser(S)
        _, C0 = eng.diagonalise(T + V, X)
        P0 = 2.0 * C0[:, :nocc] @ C0[:, :nocc].T
        nao = [sum(s.n_sph for s in shells if s.atom == k) for k in range(len(atoms))]
        r = eng.scf_rhf(S, T, V, 0.5 * (P0 + P0.T), float(np.sum(P0 * (T + V))), nocc, mol.nuclear_repulsion(atoms), X=X, conv="tight",
                        damping="dynamic", n_atom_ao=nao, max_iter=200, hfx=f["hfx"])
        C, eps, P = r["C"], r["epsilons"], r["P"]
        o, v = nocc, N - nocc
        res = {"N": N, "o": o, "v": v, "dim": o * v, "G": G, "grid": a.grid, "scf_converged": bool(r["converged"]), "scf_iterations": int(r["n_iter"]),
               "plan": Engine.xc_kernel_plan(o * v, G)}
        for _ in range(2):
            t0 = time.perf_counter()
            eng.xc_kernel_rhf(C, P, nocc, 0)
            wall = time.perf_counter() - t0
        res["xc_kernel_rhf"] = dict(eng.xc_kernel_timings(), wall_with_copies=wall)
        res["flops_k_kernel"] = 2.0 * 2 * G * (o * v) * (o * v + 64) / 2        # two matrices, the upper triangle of 64-wide blocks, 2 flops per fma
        res["baseline_torch_matmul_on_T_slabs"] = {"slab": a.slab, "seconds": baseline(G, o, v, a.slab)}
        res["k_kernel_over_baseline"] = res["xc_kernel_rhf"]["k_kernel"] / res["baseline_torch_matmul_on_T_slabs"]["seconds"]
        res["stages"] = ["wall", "MO blocks", "assembly (with the kernel build)", "solves"]
        for name, call in (("tddft_rhf TDA", lambda: eng.tddft_rhf(C, eps, P, nocc, 0, method="TDA", dip=D)),
                           ("tddft_rhf TDDFT", lambda: eng.tddft_rhf(C, eps, P, nocc, 0, method="TDDFT", dip=D)),
                           ("cis_rhf CIS", lambda: eng.cis_rhf(C, eps, nocc, 0, method="CIS", dip=D)),
                           ("cis_rhf TDHF", lambda: eng.cis_rhf(C, eps, nocc, 0, method="TDHF", dip=D))):
            try:
                for _ in range(2):
                    out = call()
                res[name] = {"seconds": out["seconds"], "lowest_singlet": float(out["E_singlet"][0]), "lowest_triplet": float(out["E_triplet"][0])}
            except TunaError as e:
                res[name] = {"refused": str(e)[:200]}
        eng.dft_clear()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
