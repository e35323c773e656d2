#!/usr/bin/env python3
"""Generate tests/golden/ump2_systems.npz: unrestricted MP2 of the REAL reference (needs oracle/_ref, `bash oracle/build_ref.sh`).

Per system: the reference's own UHF cycle from a core guess at EXTREME convergence (tools/make_golden.py, the body of
run_reference_uhf, keeping the orbitals), then the reference's run_unrestricted_MP2 (tuna_mp.py:987-1222) on its spin-blocked
tensor (tuna_ci.py:564), executed from the source text with the tuna_ci helpers it calls.  The pair energies are taken from the
return values of calculate_unrestricted_MP2_energy (E_aa, E_bb, then E_ab / 4), not from the printed lines.  Stored:
C_alpha, C_beta, eps_alpha, eps_beta, n_alpha, n_beta, E_UHF, E_aa, E_bb, E_ab; frozen-core variants with 2 and 3 frozen spin
orbitals (fc2_*, fc3_*: the reference's split, ceil(k/2) alpha and floor(k/2) beta); SCS-MP2 energies (scs_E_MP2, the default
scalings 1/3 and 6/5) where asked.  Only data is written.
"""
from __future__ import annotations

import ast
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from tuna_amd import molecule as mol  # noqa: E402

A = mol.angstrom_to_bohr
# tag -> (symbols, R in bohr or None, basis, n_alpha, n_beta, SCS run)
UMP2_SYSTEMS = {
    "o2_triplet_sto3g": (["O", "O"], A(1.2075), "STO-3G", 9, 7, False),
    "o2_triplet_ccpvdz": (["O", "O"], A(1.2075), "cc-pVDZ", 9, 7, True),
    "no_doublet_631g": (["N", "O"], A(1.1508), "6-31G", 8, 7, False),
    "oh_doublet_ccpvdz": (["O", "H"], A(0.9697), "cc-pVDZ", 5, 4, False),
    "li_doublet_631g": (["LI"], None, "6-31G", 2, 1, False),
    "h_ccpvdz": (["H"], None, "cc-pVDZ", 1, 0, False),
    "o2_triplet_ccpvtz": (["O", "O"], A(1.2075), "cc-pVTZ", 9, 7, False),
    "n2_ccpvtz": (["N", "N"], A(1.0977), "cc-pVTZ", 7, 7, True),           # closed shell: the unrestricted route of SCS-MP2
}


def load_reference_ump2():
    """run_unrestricted_MP2 and the functions it calls, from tuna_mp.py / tuna_ci.py source text; the energy helper is wrapped
    so that every pair energy it returns is recorded."""
    stubs = mg._stub_modules()["tuna_util"]
    ci = types.SimpleNamespace()
    ns_ci = {"np": np, "ndarray": np.ndarray, "Calculation": object, "log": stubs.log, "timer": stubs.timer, "error": stubs.error}
    src_ci = open(os.path.join(mg.REF, "TUNA", "tuna_ci.py")).read()
    for node in ast.parse(src_ci).body:
        if isinstance(node, ast.FunctionDef) and node.name in ("spin_block_molecular_orbitals", "transform_ERI_AO_to_SO", "antisymmetrise_integrals",
                                                                 "build_doubles_epsilons_tensor", "build_MP2_t_amplitudes"):
            exec(compile(ast.Module([node], []), "tuna_ci.py", "exec"), ns_ci)
            setattr(ci, node.name, ns_ci[node.name])
    spin_block_line = src_ci.split("\n")[563].strip()
    assert spin_block_line.startswith("ERI_spin_block = np.kron"), spin_block_line
    ns = {"np": np, "ndarray": np.ndarray, "Calculation": object, "Molecule": object, "Output": object, "ci": ci,
          "log": stubs.log, "log_spacer": stubs.log_spacer, "timer": stubs.timer, "error": stubs.error}
    lines, _ = mg._parseable_lines(os.path.join(mg.REF, "TUNA", "tuna_mp.py"))     # (logging lines Python 3.10 cannot parse become `pass`)
    for node in ast.parse("\n".join(lines)).body:
        if isinstance(node, ast.FunctionDef) and node.name in ("calculate_unrestricted_MP2_energy", "spin_component_scale_MP2_energy",
                                                               "build_t_amplitude_density_contribution", "run_unrestricted_MP2"):
            exec(compile(ast.Module([node], []), "tuna_mp.py", "exec"), ns)
    record = []
    energy = ns["calculate_unrestricted_MP2_energy"]

    def recorded(t, g):
        e = energy(t, g)
        record.append(float(e))
        return e
    ns["calculate_unrestricted_MP2_energy"] = recorded

    def spin_block(ERI_AO):
        return eval(spin_block_line.split("=", 1)[1], {"np": np, "ERI_AO": ERI_AO})
    return ns["run_unrestricted_MP2"], spin_block, record


def reference_uhf_orbitals(scf, ortho, atoms, shells, S, T, V, ERI, n_alpha, n_beta):
    """make_golden.run_reference_uhf (core guess, EXTREME, dynamic damping), keeping the orbitals of the converged cycle."""
    X, smallest, S_inv = ortho(S, None, True)
    eps0, C0 = scf.diagonalise_Fock_matrix(T + V, X)
    Pa0 = scf.construct_density_matrix(C0, n_alpha, 1)
    Pb0 = scf.construct_density_matrix(C0, n_beta, 1)
    E0 = float(np.einsum("mn,mn->", T + V, Pa0 + Pb0))
    n_sph = [sum(s.n_sph for s in shells if s.atom == a) for a in range(len(atoms))]
    molecule = types.SimpleNamespace(n_doubly_occ=n_beta, partition_ranges=n_sph, atoms=atoms, n_electrons=n_alpha + n_beta,
                                     n_alpha=n_alpha, n_beta=n_beta)
    orig = scf.format_output_line
    scf.format_output_line = lambda *a, **k: None
    try:
        calc = mg.Calc(mg.CONV["extreme"], damping=True)
        calc.reference = "UHF"
        out = scf.run_self_consistent_field_cycle(molecule, calc, mg.Ints(S, T, V, ERI), mol.nuclear_repulsion(atoms), X,
                                                  (Pa0 + Pb0, Pa0, Pb0, E0), (None, None, None, None), True)
    finally:
        scf.format_output_line = orig
    return out, X


def main():
    assert mg.orc.ref_engine() is not None, "run oracle/build_ref.sh first"
    scf = mg.load_reference_scf()
    blocks, ortho = mg.load_reference_kernel_bits()
    run_ump2, spin_block, record = load_reference_ump2()
    out = {}
    only = [a for a in sys.argv[1:] if not a.startswith("-")]
    for tag, (sym, R, basis, na, nb, scs) in UMP2_SYSTEMS.items():
        if only and tag not in only:
            continue
        atoms, shells, aos = mg.system(sym, R, basis)
        S, T, V, D, Q, E = mg.one_e_and_eri(atoms, aos)
        U = mg.reference_U(shells, blocks)
        Ss, Ts_, Vs, Es = mg.to_spherical(U, S), mg.to_spherical(U, T), mg.to_spherical(U, V), mg.eri_to_spherical(U, E)
        r, X = reference_uhf_orbitals(scf, ortho, atoms, shells, Ss, Ts_, Vs, Es, na, nb)
        N = Ss.shape[0]
        ERI_sb = spin_block(Es)
        molecule = types.SimpleNamespace(n_alpha=na, n_beta=nb, n_occ=na + nb)

        def ump2(n_frozen_spin, method="UMP2"):
            calc = types.SimpleNamespace(method=types.SimpleNamespace(name=method), DFT_calculation=False, SSS_requested=False,
                                         OSS_requested=False, same_spin_scaling=1 / 3, opposite_spin_scaling=6 / 5, relaxed_density=False,
                                         MPC_requested=False, MPC_prop=1, natural_orbitals=False)
            del record[:]
            E_MP2 = run_ump2(molecule, calc, r, 2 * N, slice(n_frozen_spin, na + nb), ERI_sb, X, True)[0]
            assert len(record) == 3, record
            return record[0], record[1], 4 * record[2], E_MP2
        d = dict(C_alpha=r.molecular_orbitals_alpha, C_beta=r.molecular_orbitals_beta, eps_alpha=r.epsilons_alpha, eps_beta=r.epsilons_beta,
                 n_alpha=na, n_beta=nb, E_UHF=r.energy)
        d["E_aa"], d["E_bb"], d["E_ab"], E_MP2 = ump2(0)
        assert abs(E_MP2 - (d["E_aa"] + d["E_bb"] + d["E_ab"])) < 1e-12
        if na + nb >= 3:
            for k in (2, 3):
                d[f"fc{k}_E_aa"], d[f"fc{k}_E_bb"], d[f"fc{k}_E_ab"], _ = ump2(k)
        if scs:
            d["scs_E_MP2"] = ump2(0, "USCS-MP2")[3]
        out[tag] = d
        print("UMP2", tag, N, "E_UHF", r.energy, "E_aa", d["E_aa"], "E_bb", d["E_bb"], "E_ab", d["E_ab"], "SCS", d.get("scs_E_MP2"), flush=True)
        del ERI_sb
    path = os.path.join(mg.GOLD, "ump2_systems.npz")
    if only and os.path.exists(path):
        z = np.load(path)
        for key in z.files:
            t, k = key.split("__", 1)
            if t not in out:
                out.setdefault(t, {})[k] = z[key]
    np.savez_compressed(path, **{f"{t}__{k}": v for t, d in out.items() for k, v in d.items()})


if __name__ == "__main__":
    main()
