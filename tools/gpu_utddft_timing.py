#!/usr/bin/env python3
"""Unrestricted TD-DFT / TDA and Kohn-Sham stability stage seconds on the synthetic diatomic (default N = 400) with LDA on the medium
grid, warm (the second call of everything), in one process.  The determinant is the converged closed-shell Kohn-Sham LDA solution of
the system (18 occupied orbitals) with 8 alpha and 10 beta orbitals frozen: (o_alpha, o_beta) = (10, 8), v = N - 18 for both spins,
dim = 18 (N - 18) -- a spin-blocked index of the size of the restricted tool's, on a reference the solves accept.
  * the kernel build of tf_xc_kernel_uhf split into psi GEMMs, densities and point kernels, K kernel and slab sum (tf_xc_kernel_timings),
    with 64 x 64 and with 64 x 128 tiles (tf_xc_kernel_spin_cols) and with the library's default; TFLOP/s count the elements p <= q only,
    not the zero padding of ragged blocks nor the lower halves of diagonal tiles;
  * the baseline for the K kernel: the same matrix (its alpha-alpha, alpha-beta and beta-beta blocks) from torch float64 matmul (rocBLAS)
    on MATERIALISED slabs of the transition densities T_s[g][(ia)] = psi_i psi_a of both spins, on orbital values and weights of the same
    shapes (random: the time does not depend on them), with the bytes a slab of the two arrays takes and what the whole arrays would;
  * tf_tddft_uhf TDA and full TD-DFT by stage, next to tf_cis_uhf CIS and TDHF on the same orbitals and windows;
  * tf_stability_rks (all-electron) and tf_stability_uks (the windows above).
A solve the library refuses (an unstable reference) is reported as such, not retried.  Prints one JSON line.
Usage: python tools/gpu_utddft_timing.py [--n 400] [--grid medium] [--slab 8192]
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
    """seconds of the three blocks of K from torch matmul on materialised T slabs of both spins, second of two passes"""
    import torch
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    psi = [torch.randn(G, o[s] + v[s], dtype=torch.float64, device=dev, generator=gen) for s in range(2)]
    u = [torch.randn(G, dtype=torch.float64, device=dev, generator=gen) for _ in range(3)]
    d = [o[s] * v[s] for s in range(2)]
    secs = []
    for _ in range(2):
        Kaa = torch.zeros(d[0], d[0], dtype=torch.float64, device=dev)
        Kab = torch.zeros(d[0], d[1], dtype=torch.float64, device=dev)
        Kbb = torch.zeros(d[1], d[1], dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for g0 in range(0, G, slab):
            T = []
            for s in range(2):
                p = psi[s][g0:g0 + slab]
                T.append((p[:, :o[s], None] * p[:, None, o[s]:]).reshape(-1, d[s]))       # [slab, d_s] in HBM
            Kaa.addmm_(T[0].T, T[0] * u[0][g0:g0 + slab, None])
            Kab.addmm_(T[0].T, T[1] * u[1][g0:g0 + slab, None])
            Kbb.addmm_(T[1].T, T[1] * u[2][g0:g0 + slab, None])
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    del psi, Kaa, Kab, Kbb
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
    nocc, nfa, nfb = 18, 8, 10
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
        o, v = (nocc - nfa, nocc - nfb), (N - nocc, N - nocc)
        da, db = o[0] * v[0], o[1] * v[1]
        plan = Engine.xc_kernel_spin_plan(da, db, G)
        res = {"N": N, "o": o, "v": v, "d_alpha": da, "d_beta": db, "dim": da + db, "G": G, "grid": a.grid, "scf_converged": bool(r["converged"]),
               "scf_iterations": int(r["n_iter"]), "plan": plan, "tile_shape": [64, plan["tile_cols"]]}
        args = (C, C, P / 2, P / 2, nocc, nocc, nfa, nfb)
        # both tile shapes, the default one last (it stays set): 64 x 64 (cols = 1) and 64 x 128 (cols = 2)
        res["useful_flops_k_kernel"] = 2.0 * G * (da + db) * (da + db + 1) / 2       # the elements p <= q, 2 flops per fma
        first = None
        for cols, name in ((1, "64x64"), (2, "64x128"), (0, "default")):
            eng.xc_kernel_spin_cols(cols)
            for _ in range(2):
                t0 = time.perf_counter()
                K = eng.xc_kernel_uhf(*args)
                wall = time.perf_counter() - t0
            first = K if first is None else first
            t = eng.xc_kernel_timings()
            res["xc_kernel_uhf " + name] = dict(t, wall_with_copies=wall, useful_tflops=res["useful_flops_k_kernel"] / t["k_kernel"] / 1e12,
                                                same_bits_as_64x64=bool(np.array_equal(K, first)))
        res["xc_kernel_uhf"] = res["xc_kernel_uhf default"]
        slab_bytes = 8 * a.slab * (da + db)
        res["baseline_torch_matmul_on_T_slabs"] = {"slab": a.slab, "seconds": baseline(G, o, v, a.slab), "T_slab_bytes": slab_bytes,
                                                   "T_whole_bytes": 8 * G * (da + db)}
        res["k_kernel_over_baseline"] = res["xc_kernel_uhf"]["k_kernel"] / res["baseline_torch_matmul_on_T_slabs"]["seconds"]
        res["stages"] = ["wall", "MO blocks", "assembly (with the kernel build)", "solves"]
        orb = (C, C, eps, eps)
        for name, call in (("tddft_uhf TDA", lambda: eng.tddft_uhf(*orb, P / 2, P / 2, nocc, nocc, nfa, nfb, method="TDA", dip=D)),
                           ("tddft_uhf TDDFT", lambda: eng.tddft_uhf(*orb, P / 2, P / 2, nocc, nocc, nfa, nfb, method="TDDFT", dip=D)),
                           ("cis_uhf CIS", lambda: eng.cis_uhf(*orb, nocc, nocc, nfa, nfb, method="CIS", dip=D)),
                           ("cis_uhf TDHF", lambda: eng.cis_uhf(*orb, nocc, nocc, nfa, nfb, method="TDHF", dip=D)),
                           ("stability_rks", lambda: eng.stability_rks(C, eps, P, nocc, 0)),
                           ("stability_uks", lambda: eng.stability_uks(*orb, P / 2, P / 2, nocc, nocc, nfa, nfb))):
            try:
                for _ in range(2):
                    out = call()
                res[name] = {"seconds": out["seconds"], "lowest": float(out["E"][0] if "E" in out else out.get("lowest", out.get("lowest_singlet")))}
            except TunaError as e:
                res[name] = {"refused": str(e)[:200]}
        eng.dft_clear()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
