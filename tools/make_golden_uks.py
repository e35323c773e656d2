#!/usr/bin/env python3
"""Generate tests/golden/uks_systems.npz: unrestricted Kohn-Sham runs of the REAL reference (needs oracle/_ref, `bash oracle/build_ref.sh`).

Per system, with the reference's own grid, basis-on-grid, spin densities, unrestricted functionals and V_XC code
(calculate_unrestricted_exchange_correlation_matrix, tuna_scf.py:665-750) and its outer loop with reference = "UHF" and DFT on
(tuna_scf.py:1292-1435, unrestricted correlation picked as at :1347-1351), from a core guess at EXTREME convergence, with and without
damping:
  * V_XC^alpha, V_XC^beta of the guess densities and their n_alpha, n_beta, E_X,alpha * DFX, E_X,beta * DFX, E_C * DFC;
  * the per-iteration table, the energy, the components and eps_alpha, eps_beta of both runs;
  * a sample of 400 grid points (points, weights, spin densities) as dft_systems.npz keeps, not whole grids.
The helpers are those of tools/make_golden.py; only data is written.
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from tuna_amd import molecule as mol  # noqa: E402

A = mol.angstrom_to_bohr
# tag -> (symbols, R in bohr or None, basis, n_alpha, n_beta, functional, grid)
UKS_SYSTEMS = {
    "o2_b3lyp_sto3g": (["O", "O"], A(1.2075), "STO-3G", 9, 7, "B3LYP", "loose"),
    "o2_svwn_sto3g": (["O", "O"], A(1.2075), "STO-3G", 9, 7, "SVWN", "loose"),
    "o2_b3lyp_ccpvdz": (["O", "O"], A(1.2075), "cc-pVDZ", 9, 7, "B3LYP", "medium"),
    "o2_svwn_ccpvdz": (["O", "O"], A(1.2075), "cc-pVDZ", 9, 7, "SVWN", "loose"),
    "no_blyp_631g": (["N", "O"], A(1.1508), "6-31G", 8, 7, "BLYP", "loose"),
    "oh_b3lypg_ccpvdz": (["O", "H"], A(0.9697), "cc-pVDZ", 5, 4, "B3LYP/G", "loose"),
    "li_svwn3_631g": (["LI"], None, "6-31G", 2, 1, "SVWN3", "loose"),
    "h_b3lyp_ccpvdz": (["H"], None, "cc-pVDZ", 1, 0, "B3LYP", "loose"),
    "nh_hfs_sto3g": (["N", "H"], A(1.036), "STO-3G", 5, 3, "HFS", "loose"),
    "nh_hfb_sto3g": (["N", "H"], A(1.036), "STO-3G", 5, 3, "HFB", "loose"),
    "nh_bvwn_sto3g": (["N", "H"], A(1.036), "STO-3G", 5, 3, "BVWN", "loose"),
    "nh_bvwn3_sto3g": (["N", "H"], A(1.036), "STO-3G", 5, 3, "BVWN3", "loose"),
    "nh_bhlyp_sto3g": (["N", "H"], A(1.036), "STO-3G", 5, 3, "BHLYP", "loose"),
    "nh_b1lyp_sto3g": (["N", "H"], A(1.036), "STO-3G", 5, 3, "B1LYP", "loose"),
    "nh_slyp_sto3g": (["N", "H"], A(1.036), "STO-3G", 5, 3, "SLYP", "loose"),
}
# (x functional, c functional, DFX, HFX, DFC, class): rows of the reference's table, tuna_util.py:1445-1475
FUN = {"B3LYP": ("B3", "3P", 0.80, 0.20, 1.0, "GGA"), "BLYP": ("B", "LYP", 1.0, 0.0, 1.0, "GGA"), "SVWN": ("S", "VWN5", 1.0, 0.0, 1.0, "LDA"),
       "B3LYP/G": ("B3", "3P", 0.80, 0.20, 1.0, "GGA"), "HFS": ("S", None, 1.0, 0.0, 0.0, "LDA"), "SVWN3": ("S", "VWN3", 1.0, 0.0, 1.0, "LDA"),
       "HFB": ("B", None, 1.0, 0.0, 0.0, "GGA"), "BVWN": ("B", "VWN5", 1.0, 0.0, 1.0, "GGA"), "BVWN3": ("B", "VWN3", 1.0, 0.0, 1.0, "GGA"),
       "BHLYP": ("B", "LYP", 0.50, 0.50, 1.0, "GGA"), "B1LYP": ("B", "LYP", 0.75, 0.25, 1.0, "GGA"), "SLYP": ("S", "LYP", 1.0, 0.0, 1.0, "GGA")}
GRID = {"loose": (3, 0.7), "medium": (4, 0.9), "tight": (5, 1.0)}            # tuna_util.py:129-137
MAX_ITER = 300                                                                 # (NO / 6-31G from the core guess without damping: 253)
LEB = np.array([3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 27, 29, 31, 35, 41, 47, 53, 59, 65, 71, 77, 83, 89, 95, 101, 107, 113, 119, 125, 131])


def run_system(scf, xc, dft, blocks, ortho, adata, sym, R, basis, na, nb, method, grid):
    atoms, shells, aos = mg.system(sym, R, basis)
    S, T, V, D, Q, E = mg.one_e_and_eri(atoms, aos)
    U = mg.reference_U(shells, blocks)
    Ss, Ts_, Vs, Es = mg.to_spherical(U, S), mg.to_spherical(U, T), mg.to_spherical(U, V), mg.eri_to_spherical(U, E)
    X, smallest, S_inv = ortho(Ss, None, True)
    xname, cname, DFX, HFX, DFC, fclass = FUN[method]
    acc, mult = GRID[grid]
    ref_atoms = [types.SimpleNamespace(real_vdw_radius=adata[a.symbol]["real_vdw_radius"], ghost=False, origin=a.origin, charge=a.charge)
                 for a in atoms]
    extent = mult * max(a.real_vdw_radius for a in ref_atoms) / 6
    leb = int(LEB[np.abs(LEB - int(acc * 9)).argmin()])
    n_radial = int(extent * acc)
    points, weights = dft.build_molecular_grid(extent, n_radial, leb, float(R or 0.0), ref_atoms)
    bfs = mg.orc.ref_basis_list(aos)
    bfs_on_grid = dft.construct_basis_functions_on_grid(bfs, points, U)
    grads = dft.construct_basis_function_gradients_on_grid(bfs, points, U) if fclass == "GGA" else None
    eps0, C0 = scf.diagonalise_Fock_matrix(Ts_ + Vs, X)                           # core guess
    Pa0, Pb0 = scf.construct_density_matrix(C0, na, 1), scf.construct_density_matrix(C0, nb, 1)
    E0 = float(np.einsum("mn,mn->", Ts_ + Vs, Pa0 + Pb0))
    x_fun = xc.exchange_functionals.get(xname)
    c_fun = xc.correlation_functionals.get(cname)
    c_fun_u = getattr(xc, c_fun.__name__.replace("restricted", "unrestricted")) if c_fun is not None else None   # tuna_scf.py:1347-1351
    runs = {}
    for damping in (True, False):
        calc = mg.Calc(mg.CONV["extreme"], damping=damping, max_iter=MAX_ITER)
        calc.reference = "UHF"
        calc.DFT_calculation = True
        calc.HFX_prop, calc.DFX_prop, calc.DFC_prop = HFX, DFX, DFC
        calc.X_alpha = 2 / 3
        calc.method = types.SimpleNamespace(name=method)
        calc.functional = types.SimpleNamespace(functional_class=fclass, x_functional=xname, c_functional=cname)
        if "xc0" not in runs:
            Va, Vb, rho_a, rho_b, rho, eXa, eXb, eC = scf.calculate_unrestricted_exchange_correlation_matrix(
                Pa0, Pb0, bfs_on_grid, grads, weights, calc, x_fun, c_fun_u)
            runs["xc0"] = dict(V_XC0_alpha=Va, V_XC0_beta=Vb, n0=np.array([np.sum(rho_a * weights), np.sum(rho_b * weights)]),
                               EX0=np.array([np.sum(eXa * rho_a * weights) * DFX, np.sum(eXb * rho_b * weights) * DFX]),
                               EC0=float(np.sum(eC * rho * weights)) * DFC if eC is not None else 0.0,
                               rho_pick=(rho_a, rho_b))
        n_sph = [sum(s.n_sph for s in shells if s.atom == a) for a in range(len(atoms))]
        molecule = types.SimpleNamespace(n_doubly_occ=nb, partition_ranges=n_sph, atoms=atoms, n_electrons=na + nb, n_alpha=na, n_beta=nb)
        table = []
        orig, saved_tab = scf.format_output_line, scf.exchange_correlation_functionals

        def rec(E_total, delta_E, max_DP, RMS_DP, damping_factor, step, commutator, calculation, silent=False):
            table.append([step, E_total, delta_E, RMS_DP, max_DP, commutator, float(damping_factor)])
        scf.format_output_line = rec
        scf.exchange_correlation_functionals = {method: calc.functional}
        try:
            o = scf.run_self_consistent_field_cycle(molecule, calc, mg.Ints(Ss, Ts_, Vs, Es), mol.nuclear_repulsion(atoms), X,
                                                    (Pa0 + Pb0, Pa0, Pb0, E0), (bfs_on_grid, weights, grads, points), True)
        finally:
            scf.format_output_line, scf.exchange_correlation_functionals = orig, saved_tab
        sfx = "" if damping else "_nodamp"
        runs[sfx] = {f"table{sfx}": np.array(table), f"energy{sfx}": o.energy, f"eps_alpha{sfx}": o.epsilons_alpha,
                     f"eps_beta{sfx}": o.epsilons_beta,
                     f"components{sfx}": np.array([o.kinetic_energy, o.nuclear_electron_energy, o.coulomb_energy, o.exchange_energy,
                                                   o.correlation_energy])}
    G = weights.size
    pick = np.random.default_rng(7).integers(0, G, 400)
    x0 = runs.pop("xc0")
    rho_a, rho_b = x0.pop("rho_pick")
    d = dict(symbols=np.array(sym), R=np.nan if R is None else float(R), basis=basis, n_alpha=na, n_beta=nb, functional=method, grid=grid,
             n_points=G, n_radial=n_radial, lebedev=leb, weights_sum=float(weights.sum()), pick=pick,
             pts_pick=points.reshape(3, -1)[:, pick], w_pick=weights.reshape(-1)[pick], rho_a_pick=rho_a.reshape(-1)[pick],
             rho_b_pick=rho_b.reshape(-1)[pick], max_iter=MAX_ITER, P0_alpha=Pa0, P0_beta=Pb0, E0=E0, **x0)
    for r in runs.values():
        d.update(r)
    return d


def main():
    assert mg.orc.ref_engine() is not None, "run oracle/build_ref.sh first"
    only = set(sys.argv[1:])
    scf = mg.load_reference_scf()
    blocks, ortho = mg.load_reference_kernel_bits()
    xc, dft, patched = mg.load_reference_dft()
    scf.dft, scf.xc = dft, xc                                       # tuna_scf.py does `import tuna_dft as dft`, `import tuna_xc as xc`
    adata = json.load(open(os.path.join(mg.ROOT, "tuna_amd", "data", "atomic_data.json")))
    out = {}
    for tag, (sym, R, basis, na, nb, method, grid) in UKS_SYSTEMS.items():
        if only and tag not in only:
            continue
        d = run_system(scf, xc, dft, blocks, ortho, adata, sym, R, basis, na, nb, method, grid)
        out[tag] = d
        print("UKS", tag, method, basis, "G", d["n_points"], "E", d["energy"], d["energy_nodamp"], "iters", len(d["table"]),
              len(d["table_nodamp"]), flush=True)
    np.savez_compressed(os.path.join(mg.GOLD, "uks_systems.npz"), **{f"{t}__{k}": v for t, d in out.items() for k, v in d.items()})


if __name__ == "__main__":
    main()
