#!/usr/bin/env python3
"""Generate tests/golden/tddft_systems.npz and tests/golden/tddft_text.json: closed-shell TD-DFT and TDA of the REAL reference for the
local-density functionals (needs oracle/_ref, `bash oracle/build_ref.sh`).

Per system: the reference's own Kohn-Sham SCF at EXTREME convergence from the core guess on its own grid (the set-up of
make_golden.make_dft_golden), then calculate_restricted_exchange_correlation_kernel_matrices (tuna_dft.py:1097-1183) and
run_excited_state_calculation (tuna_ci.py:2150-2290) with density_functional_method = True -- TDA and full TD-DFT, all-electron (fc0)
and with one frozen orbital (fc1, where o > 1) -- all executed from the source text, never copied.  Stored per system: C, eps, P,
n_occ, E_SCF, dip [3, N, N], the grid (name, n_points, n_radial, lebedev, extent), K_fc<n>_singlet / _triplet [dim, dim], and per
method (TDA, TDDFT) and window E_singlet, E_triplet (all states) and of the merged, sorted list energies, labels (0 = singlet,
1 = triplet), tdm (|mu|) and osc; 400 picked grid points (pick, pts_pick, w_pick) with the reference's density there (rho_pick) and
its f_X, f_C^singlet, f_C^triplet (fx_pick, fcs_pick, fct_pick: twice the kernels of tuna_xc.py, the factors of tuna_dft.py:1116-1124).
Where the reference drops roots (an unstable Kohn-Sham solution) only the marker <method>_fc<n>_unstable and the numbers of roots it
kept are stored, as make_golden_cis.py does.

The reference's tables have no correlation kernel for a functional without correlation: for HFS (c_functional None, DFC = 0) its
`correlation_density_kernels.get(None)` is None and the call fails.  For that one row this tool hands the reference's tables an entry
None -> zeros; DFC = 0 multiplies it away.

ladder__<HFS|VWN5|VWN3>: the same four point quantities on a density ladder of 200 logarithmically spaced values from 1e-23 to 1e3,
rows rho, f_X, f_C^singlet, f_C^triplet.  tddft_text.json: what the reference prints for `SPE : C O 1.128 : SVWN 6-31G : TD NSTATES 5`
and its `TD TDA` variant, from the first line of the kernel build to the end of the spectrum table, and the .npz the state vectors those
blocks were printed from (text_<n>_X, text_<n>_Y [n_states, o, v], in the merged order).  The kernel build is called with
DFT_calculation off, which skips only the N^2-sized contraction for K_XC_full that nothing here reads.  N2/cc-pVDZ (dim = 147) is
generated too, and dropped again when the file would exceed MAX_BYTES.  Only data is written."""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from make_golden_cis import load_reference_excited_states  # noqa: E402
from tuna_amd import guess as guess_mod  # noqa: E402
from tuna_amd import molecule as mol  # noqa: E402

A = mol.angstrom_to_bohr
# tag -> (symbols, R in bohr, basis, n_occ, functional, grid)
SYSTEMS = {
    "h2_lda_sto3g": (["H", "H"], A(0.74), "STO-3G", 1, "LDA", "loose"),
    "lih_hfs_sto3g": (["LI", "H"], A(1.595), "STO-3G", 2, "HFS", "loose"),
    "lih_svwn3_sto3g": (["LI", "H"], A(1.595), "STO-3G", 2, "SVWN3", "loose"),
    "hf_svwn_631g": (["F", "H"], A(0.917), "6-31G", 5, "SVWN", "loose"),
    "co_lda_631g": (["C", "O"], A(1.128), "6-31G", 7, "LDA", "loose"),
    "n2_lda_ccpvdz": (["N", "N"], A(1.0977), "cc-pVDZ", 7, "LDA", "loose"),
}
# (x functional, c functional, DFX, HFX, DFC): the rows of the reference's table, tuna_util.py:1445-1452
FUN = {"HFS": ("S", None, 1.0, 0.0, 0.0), "SVWN": ("S", "VWN5", 1.0, 0.0, 1.0), "LDA": ("S", "VWN5", 1.0, 0.0, 1.0), "SVWN3": ("S", "VWN3", 1.0, 0.0, 1.0)}
GRID = {"loose": (3, 0.7), "medium": (4, 0.9), "tight": (5, 1.0)}            # tuna_util.py:129-137
LEB = np.array([3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 27, 29, 31, 35, 41, 47, 53, 59, 65, 71, 77, 83, 89, 95, 101, 107, 113, 119, 125, 131])
TEXT_CASES = [("SPE : C O 1.128 : SVWN 6-31G : TD NSTATES 5", "co_lda_631g", "TDDFT", 5),
              ("SPE : C O 1.128 : SVWN 6-31G : TD TDA NSTATES 5", "co_lda_631g", "TDA", 5)]
MAX_BYTES = 450 * 1024        # "of the size of cis_systems.npz's kind" (212 KB): above this the largest system is dropped


def kohn_sham(scf, xc, dft, blocks, ortho, adata, sym, R, basis, nocc, method, grid):
    """The reference's restricted Kohn-Sham SCF at EXTREME from the core guess (the set-up of make_golden.make_dft_golden)."""
    atoms, shells, aos = mg.system(sym, R, basis)
    S, T, V, D, Q, E = mg.one_e_and_eri(atoms, aos)
    U = mg.reference_U(shells, blocks)
    Ss, Ts_, Vs, Es = mg.to_spherical(U, S), mg.to_spherical(U, T), mg.to_spherical(U, V), mg.eri_to_spherical(U, E)
    dip = np.array([mg.to_spherical(U, d) for d in D])
    X, smallest, S_inv = ortho(Ss, None, True)
    xname, cname, DFX, HFX, DFC = FUN[method]
    acc, mult = GRID[grid]
    ref_atoms = [types.SimpleNamespace(real_vdw_radius=adata[a.symbol]["real_vdw_radius"], ghost=False, origin=a.origin, charge=a.charge) for a in atoms]
    extent = mult * max(a.real_vdw_radius for a in ref_atoms) / 6
    leb = int(LEB[np.abs(LEB - int(acc * 9)).argmin()])
    n_radial = int(extent * acc)
    points, weights = dft.build_molecular_grid(extent, n_radial, leb, float(R), ref_atoms)
    bfs_on_grid = dft.construct_basis_functions_on_grid(mg.orc.ref_basis_list(aos), points, U)
    eps0, C0 = scf.diagonalise_Fock_matrix(Ts_ + Vs, X)
    P0 = scf.construct_density_matrix(C0, nocc, 2)
    E0 = float(np.einsum("mn,mn->", Ts_ + Vs, P0))
    calc = mg.Calc(mg.CONV["extreme"], damping=True)
    calc.DFT_calculation = True
    calc.HFX_prop, calc.DFX_prop, calc.DFC_prop = HFX, DFX, DFC
    calc.X_alpha = 2 / 3
    calc.method = types.SimpleNamespace(name=method)
    calc.functional = types.SimpleNamespace(functional_class="LDA", x_functional=xname, c_functional=cname, time_dependent_available=True)
    saved_tab = scf.exchange_correlation_functionals
    scf.exchange_correlation_functionals = {method: calc.functional}
    n_sph = [sum(s.n_sph for s in shells if s.atom == a) for a in range(len(atoms))]
    molecule = types.SimpleNamespace(n_doubly_occ=nocc, partition_ranges=n_sph, atoms=atoms, n_electrons=2 * nocc, n_alpha=nocc, n_beta=nocc)
    orig = scf.format_output_line
    scf.format_output_line = lambda *a, **k: None
    try:
        o = scf.run_self_consistent_field_cycle(molecule, calc, mg.Ints(Ss, Ts_, Vs, Es), mol.nuclear_repulsion(atoms), X, (P0, P0 / 2, P0 / 2, E0),
                                                (bfs_on_grid, weights, None, points), True)
    finally:
        scf.format_output_line = orig
        scf.exchange_correlation_functionals = saved_tab
    return dict(atoms=atoms, Es=Es, dip=dip, out=o, calc=calc, bfs_on_grid=bfs_on_grid, weights=weights, points=points,
                grid=dict(n_points=weights.size, n_radial=n_radial, lebedev=leb, extent=extent))


def point_quantities(xc, calc, rho):
    """rho (floored as the reference's density is), f_X, f_C^singlet, f_C^triplet by the reference's kernels and factors"""
    n = np.maximum(np.asarray(rho, float), 1e-23)
    f = calc.functional
    zero = np.zeros_like(n)
    fx = 2 * xc.exchange_kernels[f.x_functional](n, None, None, calc) if f.x_functional else zero
    fcs = 2 * xc.correlation_density_kernels[f.c_functional](n, None, None, calc) if f.c_functional else zero
    fct = 2 * xc.correlation_spin_kernels[f.c_functional](n, None, None, calc) if f.c_functional else zero
    return np.array([n, fx, fcs, fct])


def main():
    assert mg.orc.ref_engine() is not None, "run oracle/build_ref.sh first"
    blocks, ortho = mg.load_reference_kernel_bits()
    scf = mg.load_reference_scf()
    xc, dft, patched = mg.load_reference_dft()
    scf.dft, scf.xc = dft, xc
    ns, stream, seen = load_reference_excited_states()
    dft.log = ns["log"]                                    # the three lines of the kernel build go to the same stream
    for table in (xc.correlation_density_kernels, xc.correlation_spin_kernels):
        table[None] = lambda density, sigma, tau, calculation: np.zeros_like(density)      # HFS: see the docstring
    build_K = dft.calculate_restricted_exchange_correlation_kernel_matrices

    def build_K_seen(*a, **k):
        seen["text_start"] = len(stream)
        r = build_K(*a, **k)
        seen["K_singlet"], seen["K_triplet"] = r[0], r[1]
        return r
    ns["calculate_restricted_exchange_correlation_kernel_matrices"] = build_K_seen
    header = ns["print_initial_excited_state_information"]

    def header_only(*a, **k):                              # (make_golden_cis marks the start of the text here: TD-DFT starts earlier)
        start = seen.get("text_start")
        header(*a, **k)
        if start is not None:
            seen["text_start"] = start
    ns["print_initial_excited_state_information"] = header_only
    adata = json.load(open(os.path.join(mg.ROOT, "tuna_amd", "data", "atomic_data.json")))
    out, texts = {}, []
    for tag, (sym, R, basis, nocc, method, grid) in SYSTEMS.items():
        ks = kohn_sham(scf, xc, dft, blocks, ortho, adata, sym, R, basis, nocc, method, grid)
        o, calc0 = ks["out"], ks["calc"]
        C, eps, P, E_SCF = o.molecular_orbitals, o.epsilons, o.P, float(o.energy)
        N = len(eps)
        G = ks["weights"].size
        pick = np.random.default_rng(5).integers(0, G, 400)
        flat_density = np.asarray(o.density).reshape(-1)
        d = dict(C=C, eps=eps, P=P, n_occ=nocc, E_SCF=E_SCF, dip=ks["dip"], functional=np.array(method), grid=np.array(grid), pick=pick,
                 pts_pick=ks["points"].reshape(3, -1)[:, pick], w_pick=ks["weights"].reshape(-1)[pick], **ks["grid"])
        pq = point_quantities(xc, calc0, flat_density[pick])
        d.update(rho_pick=pq[0], fx_pick=pq[1], fcs_pick=pq[2], fct_pick=pq[3])
        com = guess_mod.centre_of_mass(ks["atoms"]) if len(ks["atoms"]) == 2 else 0.0
        xname, cname, DFX, HFX, DFC = FUN[method]

        def run(tda, nf, n_states=10, root=1):
            calc = types.SimpleNamespace(method=types.SimpleNamespace(name=method, density_functional_method=True, excited_state_method=False),
                                         tamm_dancoff_approximation=tda, calculate_no_singlets=False, calculate_no_triplets=False, reference="RHF",
                                         HFX_prop=HFX, DFX_prop=DFX, DFC_prop=DFC, X_alpha=2 / 3, DFT_calculation=False, root=root, n_states=n_states,
                                         excited_state_contribution_threshold=1.0, freeze_core=nf > 0, do_perturbative_doubles=False,
                                         plot_absorbance_spectrum=False, functional=calc0.functional, time_dependent=True)
            molecule = types.SimpleNamespace(n_core_orbitals=nf, n_electrons=2 * nocc, n_doubly_occ=nocc, n_doubly_virt=N - nocc, centre_of_mass=com)
            scf_out = types.SimpleNamespace(integrals=types.SimpleNamespace(ERI_AO=ks["Es"]), molecular_orbitals=C, epsilons=eps, D=ks["dip"], P=P,
                                            P_alpha=P / 2, P_beta=P / 2, energy=E_SCF, density=o.density)
            stream.clear(); seen.clear()
            state = ns["run_excited_state_calculation"](molecule, calc, scf_out, ks["bfs_on_grid"], ks["weights"], False)
            dim = (nocc - nf) * (N - nocc)
            K = dict(singlet=np.array(seen["K_singlet"]).reshape(dim, dim), triplet=np.array(seen["K_triplet"]).reshape(dim, dim))
            if seen.get("warnings") or len(seen["E_singlet"]) != dim or len(seen["E_triplet"]) != dim:
                assert not tda, (tag, tda, nf, seen.get("warnings"))
                return K, dict(unstable=1, n_real_singlet=len(seen["E_singlet"]), n_real_triplet=len(seen["E_triplet"]))
            assert abs(state[0] - (E_SCF + seen["energies"][root - 1])) < 1e-12
            return K, dict(E_singlet=np.array(seen["E_singlet"]), E_triplet=np.array(seen["E_triplet"]), energies=np.array(seen["energies"]),
                           labels=np.array([0 if s == "singlet" else 1 for s in seen["labels"]], dtype=np.uint8), tdm=np.array(seen["tdm"], dtype=float),
                           osc=np.array(seen["osc"], dtype=float))
        for nf in ((0, 1) if nocc > 1 else (0,)):
            for name, tda in (("TDA", True), ("TDDFT", False)):
                K, r = run(tda, nf)
                d.update({f"K_fc{nf}_{m}": K[m] for m in K})
                d.update({f"{name}_fc{nf}_{k}": val for k, val in r.items()})
                if "unstable" in r:
                    print("TDDFT", tag, name, f"fc{nf}", "UNSTABLE reference: no golden", r, flush=True)
                    continue
                print("TDDFT", tag, method, name, f"fc{nf}", "dim", len(r["E_singlet"]), "lowest singlet", r["E_singlet"][0], "lowest triplet",
                      r["E_triplet"][0], "sum f", r["osc"].sum(), "|K_S|", np.abs(K["singlet"]).max(), flush=True)
        for n, (line, system, name, n_states) in enumerate(TEXT_CASES):
            if system != tag:
                continue
            run(name == "TDA", 0, n_states=n_states)
            ov = seen["n_occ"] * seen["n_virt"]
            vec = seen["vectors"][:, :n_states]
            X = vec[:ov].T.reshape(n_states, seen["n_occ"], seen["n_virt"])
            Y = vec[ov:].T.reshape(X.shape) if vec.shape[0] == 2 * ov else np.zeros_like(X)
            d[f"text_{n}_X"], d[f"text_{n}_Y"] = X, Y
            texts.append(dict(line=line, system=system, method=name, n_states=n_states, prefix=f"{name}_fc0_", vectors=f"text_{n}_",
                              text="".join(stream[seen["text_start"]:])))
        out[tag] = d
    ladder = np.logspace(-23, 3, 200)
    for name, (xn, cn) in (("HFS", ("S", None)), ("VWN5", (None, "VWN5")), ("VWN3", (None, "VWN3"))):
        calc = types.SimpleNamespace(X_alpha=2 / 3, functional=types.SimpleNamespace(x_functional=xn, c_functional=cn))
        out.setdefault("ladder", {})[name] = point_quantities(xc, calc, ladder)

    def flat(systems):
        return {f"{t}__{k}": v for t, dd in systems.items() for k, v in dd.items()}
    path = os.path.join(mg.GOLD, "tddft_systems.npz")
    np.savez_compressed(path, **flat(out))
    if os.path.getsize(path) > MAX_BYTES:
        print(f"tddft_systems.npz would be {os.path.getsize(path)} bytes: dropping n2_lda_ccpvdz", flush=True)
        out.pop("n2_lda_ccpvdz")
        np.savez_compressed(path, **flat(out))
    print("tddft_systems.npz:", os.path.getsize(path), "bytes, systems", [t for t in out if t != "ladder"])
    with open(os.path.join(mg.GOLD, "tddft_text.json"), "w") as f:
        json.dump(texts, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
