#!/usr/bin/env python3
"""Generate tests/golden/utddft_systems.npz and tests/golden/utddft_text.json: unrestricted TD-DFT / TDA and the Kohn-Sham stability
analysis of the REAL reference for the local-density functionals (needs oracle/_ref, `bash oracle/build_ref.sh`).

Open shells.  Per system the reference's own unrestricted Kohn-Sham SCF at EXTREME convergence from the core guess on its own grid (the
set-up of make_golden_uks.py), then calculate_unrestricted_exchange_correlation_kernel_matrices (tuna_dft.py:1194-1281),
run_excited_state_calculation on its "UHF" branch with density_functional_method on (tuna_ci.py:2215-2290) -- TDA and full TD-DFT, all-
electron (fc0) and with one frozen orbital per spin (fc2, where o_beta > 1) -- and determine_self_consistent_field_stability
(:1049-1106), all executed from the source text, never copied.  Stored per system: C_alpha, C_beta, eps_alpha, eps_beta, P_alpha, P_beta,
n_alpha, n_beta, E_SCF, dip [3, N, N], the grid (name, n_points, n_radial, lebedev, extent), K_fc<k> [dim, dim] -- the reference's K_XC
restricted to the spin-conserving excitations and permuted to the library's order (alpha block (ia) = i v_a + a, then beta) --, per
method (TDA, TDDFT) and window energies, tdm (|mu|) and osc, stab_fc<k>_lowest (the lowest eigenvalue of the reference's Hessian), and
400 picked grid points (pick, pts_pick, w_pick) with the reference's spin densities there (rho_a_pick, rho_b_pick) and its five point
kernels (fxaa_pick, fxbb_pick, fcaa_pick, fcab_pick, fcbb_pick: the factors of tuna_dft.py:1243-1248).  Where the reference's Hessian
is not positive definite (UNSTABLE_BELOW, ZERO_MODE_BELOW of make_golden_ucis.py) or it drops roots, only the marker
<method>_fc<k>_unstable / _marginal is stored: such a system is compared on K and the stability eigenvalue only.

The two conditions of make_golden_ucis.py tie the reference's energy-sorted spin orbitals to the library's windows and are asserted
here; a system that does not meet them is dropped with a message.  At least four systems must be stable, cover HFS, VWN3 and VWN5
between them and include one with o_beta <= 1: asserted.

O2/STO-3G SVWN (9, 7) from the core guess fails the first condition (the reference occupies another determinant than the windows name) and
is dropped.  OH and NO in 6-31G with LDA do not converge in the reference's own cycle from the core guess within 300 iterations and are
not listed; OH/STO-3G stands in as the VWN5 doublet with a frozen variant.  H/6-31G (1, 0) runs: its beta block is empty.

Unstable solutions: LiH at 4.0 angstrom (2, 2) and H2 at 3.0 angstrom (1, 1), whose unrestricted cycle from the core guess stays on the
spin-restricted solution beyond the point where it breaks spin symmetry: the reference's Hessian has the eigenvalues -0.078 and -0.146,
and only K, the eigenvalue and the unstable markers are stored.

The reference's tables have no correlation kernel for a functional without correlation (HFS): this tool hands them an entry
None -> zeros, as make_golden_tddft.py does; DFC = 0 multiplies it away.

ladder__<HFS|VWN5|VWN3>: the seven point quantities (rho_a, rho_b, f_X,aa, f_X,bb, f_C,aa, f_C,ab, f_C,bb) on pairs (rho_a, rho_b): total
densities from 1e-20 to 1e3 at zeta = 0, +-0.3, +-0.9, +-(1 - 1e-9), +-1 (the other spin exactly at the floor), and both spins at the floor.

Closed shells: rks__<tag>__singlet / triplet, the lowest eigenvalues of the reference's singlet and triplet Kohn-Sham Hessians for the
systems of tests/golden/tddft_systems.npz, recomputed from their stored C, eps and P on the reference's grid.

utddft_text.json: what the reference prints for one TD and one TD TDA run (from the first line of the kernel build to the end of the
spectrum table, 5 states) and for one unrestricted and one restricted STAB run; the .npz holds the vectors the excited-state blocks were
printed from in the library's order (text_<n>_X, text_<n>_Y [n_states, dim]).  Only data is written."""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
import make_golden_tddft as mt  # noqa: E402
import make_golden_ucis as mu  # noqa: E402
from make_golden_uks import FUN, GRID, LEB  # noqa: E402
from tuna_amd import guess as guess_mod  # noqa: E402
from tuna_amd import molecule as mol  # noqa: E402

A = mol.angstrom_to_bohr
# tag -> (symbols, R in bohr or None, basis, n_alpha, n_beta, functional, grid)
SYSTEMS = {
    "o2_svwn_sto3g": (["O", "O"], A(1.2075), "STO-3G", 9, 7, "SVWN", "loose"),
    "nh_hfs_sto3g": (["N", "H"], A(1.036), "STO-3G", 5, 3, "HFS", "loose"),
    "nh_svwn3_sto3g": (["N", "H"], A(1.036), "STO-3G", 5, 3, "SVWN3", "loose"),
    "li_svwn3_631g": (["LI"], None, "6-31G", 2, 1, "SVWN3", "loose"),
    "oh_lda_sto3g": (["O", "H"], A(0.9697), "STO-3G", 5, 4, "SVWN", "loose"),
    "lih_cation_lda_631g": (["LI", "H"], A(1.595), "6-31G", 2, 1, "SVWN", "loose"),
    "h_lda_631g": (["H"], None, "6-31G", 1, 0, "SVWN", "loose"),
    "lih_stretched_lda_sto3g": (["LI", "H"], A(4.0), "STO-3G", 2, 2, "SVWN", "loose"),
    "h2_stretched_svwn3_sto3g": (["H", "H"], A(3.0), "STO-3G", 1, 1, "SVWN3", "loose"),
}
TEXT_EXCITED = [("nh_hfs_sto3g", "TDDFT", 5), ("nh_hfs_sto3g", "TDA", 5)]
TEXT_STAB_U, TEXT_STAB_R = "nh_hfs_sto3g", "hf_svwn_631g"
MAX_BYTES = 450 * 1024
MAX_ITER = 300


def build_grid(dft, adata, atoms, R, grid):
    acc, mult = GRID[grid]
    ref_atoms = [types.SimpleNamespace(real_vdw_radius=adata[a.symbol]["real_vdw_radius"], ghost=False, origin=a.origin, charge=a.charge) for a in atoms]
    extent = mult * max(a.real_vdw_radius for a in ref_atoms) / 6
    leb = int(LEB[np.abs(LEB - int(acc * 9)).argmin()])
    n_radial = int(extent * acc)
    points, weights = dft.build_molecular_grid(extent, n_radial, leb, float(R or 0.0), ref_atoms)
    return points, weights, dict(n_points=weights.size, n_radial=n_radial, lebedev=leb, extent=extent)


def unrestricted_kohn_sham(scf, xc, dft, blocks, ortho, adata, sym, R, basis, na, nb, method, grid):
    """The reference's unrestricted Kohn-Sham SCF at EXTREME from the core guess (the set-up of make_golden_uks.run_system)."""
    atoms, shells, aos = mg.system(sym, R, basis)
    S, T, V, D, Q, E = mg.one_e_and_eri(atoms, aos)
    U = mg.reference_U(shells, blocks)
    Ss, Ts_, Vs, Es = mg.to_spherical(U, S), mg.to_spherical(U, T), mg.to_spherical(U, V), mg.eri_to_spherical(U, E)
    dip = np.array([mg.to_spherical(U, d) for d in D])
    X, smallest, S_inv = ortho(Ss, None, True)
    xname, cname, DFX, HFX, DFC, fclass = FUN[method]
    points, weights, gd = build_grid(dft, adata, atoms, R, grid)
    bfs_on_grid = dft.construct_basis_functions_on_grid(mg.orc.ref_basis_list(aos), points, U)
    eps0, C0 = scf.diagonalise_Fock_matrix(Ts_ + Vs, X)
    Pa0, Pb0 = scf.construct_density_matrix(C0, na, 1), scf.construct_density_matrix(C0, nb, 1)
    E0 = float(np.einsum("mn,mn->", Ts_ + Vs, Pa0 + Pb0))
    calc = mg.Calc(mg.CONV["extreme"], damping=True, max_iter=MAX_ITER)
    calc.reference = "UHF"
    calc.DFT_calculation = True
    calc.HFX_prop, calc.DFX_prop, calc.DFC_prop = HFX, DFX, DFC
    calc.X_alpha = 2 / 3
    calc.method = types.SimpleNamespace(name=method)
    calc.functional = types.SimpleNamespace(functional_class=fclass, x_functional=xname, c_functional=cname, time_dependent_available=True)
    n_sph = [sum(s.n_sph for s in shells if s.atom == a) for a in range(len(atoms))]
    molecule = types.SimpleNamespace(n_doubly_occ=nb, partition_ranges=n_sph, atoms=atoms, n_electrons=na + nb, n_alpha=na, n_beta=nb)
    orig, saved_tab = scf.format_output_line, scf.exchange_correlation_functionals
    scf.format_output_line = lambda *a, **k: None
    scf.exchange_correlation_functionals = {method: calc.functional}
    try:
        o = scf.run_self_consistent_field_cycle(molecule, calc, mg.Ints(Ss, Ts_, Vs, Es), mol.nuclear_repulsion(atoms), X, (Pa0 + Pb0, Pa0, Pb0, E0),
                                                (bfs_on_grid, weights, None, points), True)
    finally:
        scf.format_output_line, scf.exchange_correlation_functionals = orig, saved_tab
    return dict(atoms=atoms, Es=Es, dip=dip, out=o, calc=calc, bfs_on_grid=bfs_on_grid, weights=weights, points=points, grid=gd)


def point_quantities(xc, calc, rho_a, rho_b):
    """rho_a, rho_b (floored per spin as the reference's densities are) and the five kernels by the reference's functions and factors"""
    ra, rb = np.maximum(np.asarray(rho_a, float), 1e-23), np.maximum(np.asarray(rho_b, float), 1e-23)
    f = calc.functional
    zero = np.zeros_like(ra)
    xk = xc.exchange_kernels.get(f.x_functional)
    fxa = 2 * xk(2 * ra, None, None, calc) if xk else zero
    fxb = 2 * xk(2 * rb, None, None, calc) if xk else zero
    with np.errstate(all="ignore"):
        fc = xc.unrestricted_correlation_kernels[f.c_functional](ra, rb, ra + rb, None, None, None, None, None, calc) if f.c_functional else (zero, zero, zero)
    return np.array([ra, rb, fxa, fxb, fc[0], fc[1], fc[2]])


def ladder_pairs():
    n = np.logspace(-20, 3, 24)
    pairs = [(1e-23, 1e-23)]
    for z in (0.0, 0.3, -0.3, 0.9, -0.9, 1 - 1e-9, -(1 - 1e-9)):
        pairs += [(x * (1 + z) / 2, x * (1 - z) / 2) for x in n]
    pairs += [(x, 1e-23) for x in n] + [(1e-23, x) for x in n] + [(x, 0.0) for x in n[::6]]
    return np.array(pairs).T


def main():
    assert mg.orc.ref_engine() is not None, "run oracle/build_ref.sh first"
    only = set(sys.argv[1:])
    blocks, ortho = mg.load_reference_kernel_bits()
    scf = mg.load_reference_scf()
    xc, dft, patched = mg.load_reference_dft()
    scf.dft, scf.xc = dft, xc
    ns, stream, seen = mu.load_reference()
    dft.log = ns["log"]                                    # the three lines of the kernel build go to the same stream
    xc.unrestricted_correlation_kernels[None] = lambda a, b, n, *rest: (np.zeros_like(n), np.zeros_like(n), np.zeros_like(n))     # HFS: see the docstring
    for table in (xc.correlation_density_kernels, xc.correlation_spin_kernels):
        table[None] = lambda density, sigma, tau, calculation: np.zeros_like(density)
    build_K = dft.calculate_unrestricted_exchange_correlation_kernel_matrices

    def build_K_seen(*a, **k):
        seen["text_start"] = len(stream)
        r = build_K(*a, **k)
        seen["K"] = r
        return r
    ns["calculate_unrestricted_exchange_correlation_kernel_matrices"] = build_K_seen
    ns["calculate_restricted_exchange_correlation_kernel_matrices"] = dft.calculate_restricted_exchange_correlation_kernel_matrices
    contributions = ns["print_excited_state_contributions"]

    def contributions_seen(*a, **k):                       # (make_golden_ucis marks the start of the text here: TD-DFT starts earlier)
        start = seen.get("text_start")
        r = contributions(*a, **k)
        if start is not None:
            seen["text_start"] = start
        return r
    ns["print_excited_state_contributions"] = contributions_seen
    adata = json.load(open(os.path.join(mg.ROOT, "tuna_amd", "data", "atomic_data.json")))
    out, texts, n_text, stable = {}, [], 0, []
    for tag, (sym, R, basis, na, nb, method, grid) in SYSTEMS.items():
        if only and tag not in only:
            continue
        try:
            ks = unrestricted_kohn_sham(scf, xc, dft, blocks, ortho, adata, sym, R, basis, na, nb, method, grid)
        except Exception as e:                             # (the reference's own cycle cannot run this system: dropped, said so)
            print("UTDDFT", tag, "DROPPED: the reference's unrestricted Kohn-Sham cycle failed:", repr(e), flush=True)
            continue
        o, calc0 = ks["out"], ks["calc"]
        Ca, Cb, ea, eb = o.molecular_orbitals_alpha, o.molecular_orbitals_beta, o.epsilons_alpha, o.epsilons_beta
        Pa, Pb, E_SCF = o.P_alpha, o.P_beta, float(o.energy)
        N = len(ea)
        xname, cname, DFX, HFX, DFC, fclass = FUN[method]
        order = np.argsort(np.append(ea, eb))
        spins = np.array(["a"] * N + ["b"] * N)[order]
        variants = (0, 2) if nb > 1 else (0,)
        if int(np.sum(spins[:na + nb] == "a")) != na or any(int(np.sum(spins[:k] == "a")) != k // 2 for k in variants):
            print("UTDDFT", tag, "DROPPED: the lowest spin orbitals are not n_alpha alpha + n_beta beta, or the frozen ones do not split evenly", flush=True)
            continue
        G = ks["weights"].size
        pick = np.random.default_rng(9).integers(0, G, 400)
        rho_a = np.asarray(dft.construct_density_on_grid(Pa, ks["bfs_on_grid"])).reshape(-1)
        rho_b = np.asarray(dft.construct_density_on_grid(Pb, ks["bfs_on_grid"])).reshape(-1)
        pq = point_quantities(xc, calc0, rho_a[pick], rho_b[pick])
        d = dict(C_alpha=Ca, C_beta=Cb, eps_alpha=ea, eps_beta=eb, P_alpha=Pa, P_beta=Pb, n_alpha=na, n_beta=nb, E_SCF=E_SCF, dip=ks["dip"],
                 functional=np.array(method), grid=np.array(grid), pick=pick, pts_pick=ks["points"].reshape(3, -1)[:, pick],
                 w_pick=ks["weights"].reshape(-1)[pick], rho_a_pick=pq[0], rho_b_pick=pq[1], fxaa_pick=pq[2], fxbb_pick=pq[3], fcaa_pick=pq[4],
                 fcab_pick=pq[5], fcbb_pick=pq[6], **ks["grid"])
        com = guess_mod.centre_of_mass(ks["atoms"]) if len(ks["atoms"]) == 2 else 0.0
        scf_out = types.SimpleNamespace(integrals=types.SimpleNamespace(ERI_AO=ks["Es"]), molecular_orbitals_alpha=Ca, molecular_orbitals_beta=Cb,
                                        epsilons_alpha=ea, epsilons_beta=eb, epsilons_combined=np.append(ea, eb), D=ks["dip"], P=Pa + Pb, P_alpha=Pa,
                                        P_beta=Pb, energy=E_SCF)

        def molecule_ns(k):
            return types.SimpleNamespace(n_core_spin_orbitals=k, n_core_orbitals=k // 2, n_electrons=na + nb, n_occ=na + nb, n_virt=2 * N - na - nb,
                                         centre_of_mass=com)

        def calculation(k, tda, n_states=10):
            return types.SimpleNamespace(method=types.SimpleNamespace(name=method, density_functional_method=True, excited_state_method=False,
                                                                      unrestricted_available=True),
                                         tamm_dancoff_approximation=tda, calculate_no_singlets=False, calculate_no_triplets=False, reference="UHF",
                                         HFX_prop=HFX, DFX_prop=DFX, DFC_prop=DFC, X_alpha=2 / 3, DFT_calculation=False, root=1, n_states=n_states,
                                         excited_state_contribution_threshold=1.0, freeze_core=k > 0, do_perturbative_doubles=False,
                                         plot_absorbance_spectrum=False, functional=calc0.functional, time_dependent=True)

        def rows_of(k):
            return mu.library_order(seen["spin_orbital_labels"], na + nb - k, 2 * N - na - nb, ((na, k // 2), (nb, k // 2)), N)

        def run(tda, k, n_states=10):
            stream.clear(); seen.clear()
            state = ns["run_excited_state_calculation"](molecule_ns(k), calculation(k, tda, n_states), scf_out, ks["bfs_on_grid"], ks["weights"], False)
            dim = (na - k // 2) * (N - na) + (nb - k // 2) * (N - nb)
            full = (na + nb - k) * (2 * N - na - nb)
            rows = rows_of(k)
            Kfull = np.asarray(seen["K"]).reshape(full, full)
            K = Kfull[np.ix_(rows, rows)]
            if seen.get("warnings") or len(seen["energies"]) != dim:
                assert not tda, (tag, tda, k, seen.get("warnings"))
                return K, dict(unstable=1, n_real=len(seen["energies"]))
            assert abs(state[0] - (E_SCF + seen["energies"][0])) < 1e-12
            return K, dict(energies=np.array(seen["energies"]), tdm=np.array(seen["tdm"], dtype=float), osc=np.array(seen["osc"], dtype=float))
        ok = True
        for k in variants:
            stream.clear(); seen.clear()
            ns["determine_self_consistent_field_stability"](molecule_ns(k), calculation(k, False), ks["Es"], scf_out, ks["bfs_on_grid"], ks["weights"], False)
            assert len(seen["hessian_lowest"]) == 1
            lowest = d[f"stab_fc{k}_lowest"] = seen["hessian_lowest"][0]
            print("USTAB", tag, f"fc{k}", lowest, flush=True)
            if k == 0 and tag == TEXT_STAB_U:
                texts.append(dict(kind="stability", system=tag, reference="UHF", functional=method, lowest=[lowest], text=mu.stability_block(stream)))
            for name, tda in (("TDA", True), ("TDDFT", False)):
                K, r = run(tda, k)
                d[f"K_fc{k}"] = K
                if lowest <= mu.UNSTABLE_BELOW:
                    r = dict(unstable=1, n_real=r.get("n_real", len(r.get("energies", ()))))
                elif lowest < mu.ZERO_MODE_BELOW:
                    r = dict(marginal=1, n_real=r.get("n_real", len(r.get("energies", ()))))
                d.update({f"{name}_fc{k}_{key}": val for key, val in r.items()})
                if "energies" not in r:
                    ok = False
                    print("UTDDFT", tag, name, f"fc{k}", "no golden", r, flush=True)
                else:
                    print("UTDDFT", tag, method, name, f"fc{k}", "dim", len(r["energies"]), "lowest", r["energies"][0], "sum f", r["osc"].sum(), "|K|",
                          np.abs(K).max(), flush=True)
        if ok:
            stable.append((tag, method, nb))
        for system, name, n_states in TEXT_EXCITED:
            if system != tag or not ok:
                continue
            run(name == "TDA", 0, n_states)
            text = "".join(stream[seen["text_start"]:])
            rows = rows_of(0)
            full = (na + nb) * (2 * N - na - nb)
            vec = seen["vectors"][:, :n_states]
            X = vec[:full][rows].T
            Y = vec[full:][rows].T if vec.shape[0] == 2 * full else np.zeros_like(X)
            assert abs(np.sum(vec[:full] ** 2) - np.sum(X ** 2)) < 1e-12
            d[f"text_{n_text}_X"], d[f"text_{n_text}_Y"] = X, Y
            texts.append(dict(kind="excited", system=tag, method=name, functional=method, n_states=n_states, prefix=f"{name}_fc0_", vectors=f"text_{n_text}_",
                              labels=seen["spin_orbital_labels"], text=text))
            n_text += 1
        out[tag] = d
    if not only:
        funs = {FUN[m][1] for _, m, _ in stable}
        assert len(stable) >= 4 and funs >= {None, "VWN3", "VWN5"} and any(nb <= 1 for _, _, nb in stable), stable
    # ---- the ladder
    pairs = ladder_pairs()
    for name, (xn, cn) in (("HFS", ("S", None)), ("VWN5", (None, "VWN5")), ("VWN3", (None, "VWN3"))):
        calc = types.SimpleNamespace(X_alpha=2 / 3, functional=types.SimpleNamespace(x_functional=xn, c_functional=cn))
        out.setdefault("ladder", {})[name] = point_quantities(xc, calc, pairs[0], pairs[1])
    # ---- closed shells: the restricted Kohn-Sham stability numbers of the systems of tddft_systems.npz
    zt = np.load(os.path.join(mg.GOLD, "tddft_systems.npz"))
    rks = {}
    for tag, (sym, R, basis, nocc, method, grid) in mt.SYSTEMS.items():
        if f"{tag}__C" not in zt.files or (only and tag not in only):
            continue
        atoms, shells, aos = mg.system(sym, R, basis)
        S, T, V, D, Q, E = mg.one_e_and_eri(atoms, aos)
        U = mg.reference_U(shells, blocks)
        Es = mg.eri_to_spherical(U, E)
        C, eps, P, E_SCF = zt[f"{tag}__C"], zt[f"{tag}__eps"], zt[f"{tag}__P"], float(zt[f"{tag}__E_SCF"])
        N = len(eps)
        points, weights, gd = build_grid(dft, adata, atoms, R, grid)
        assert gd["n_points"] == int(zt[f"{tag}__n_points"])
        bfs_on_grid = dft.construct_basis_functions_on_grid(mg.orc.ref_basis_list(aos), points, U)
        xname, cname, DFX, HFX, DFC = mt.FUN[method]
        calc = types.SimpleNamespace(method=types.SimpleNamespace(name=method, density_functional_method=True, excited_state_method=False),
                                     tamm_dancoff_approximation=False, reference="RHF", HFX_prop=HFX, DFX_prop=DFX, DFC_prop=DFC, X_alpha=2 / 3,
                                     DFT_calculation=False, freeze_core=False,
                                     functional=types.SimpleNamespace(functional_class="LDA", x_functional=xname, c_functional=cname, time_dependent_available=True))
        molecule = types.SimpleNamespace(n_core_orbitals=0, n_electrons=2 * nocc, n_doubly_occ=nocc, n_doubly_virt=N - nocc)
        scf_out = types.SimpleNamespace(integrals=types.SimpleNamespace(ERI_AO=Es), molecular_orbitals=C, epsilons=eps, energy=E_SCF, P=P,
                                        density=dft.construct_density_on_grid(P, bfs_on_grid))
        Ei = np.ascontiguousarray(Es.transpose(0, 2, 1, 3))       # (make_golden_ucis.py: the restricted transformation's index order)
        stream.clear(); seen.clear()
        ns["determine_self_consistent_field_stability"](molecule, calc, Ei, scf_out, bfs_on_grid, weights, False)
        assert len(seen["hessian_lowest"]) == 2
        rks[f"{tag}__singlet"], rks[f"{tag}__triplet"] = seen["hessian_lowest"]
        print("RKS STAB", tag, method, seen["hessian_lowest"], flush=True)
        if tag == TEXT_STAB_R:
            texts.append(dict(kind="stability", system=tag, reference="RHF", functional=method, lowest=list(seen["hessian_lowest"]),
                              text=mu.stability_block(stream)))
    data = {f"{t}__{k}": v for t, dd in out.items() for k, v in dd.items()}
    data.update({f"rks__{k}": v for k, v in rks.items()})
    path = os.path.join(mg.GOLD, "utddft_systems.npz")
    np.savez_compressed(path, **data)
    size = os.path.getsize(path)
    print("utddft_systems.npz:", size, "bytes, systems", [t for t in out if t != "ladder"], "stable", stable)
    assert size <= MAX_BYTES, size
    with open(os.path.join(mg.GOLD, "utddft_text.json"), "w") as f:
        json.dump(texts, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
