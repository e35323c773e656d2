#!/usr/bin/env python3
"""Generate tests/golden/cis_systems.npz and tests/golden/cis_text.json: closed-shell CIS and TDHF of the REAL reference (needs
oracle/_ref, `bash oracle/build_ref.sh`).

Per system of tests/golden/mp3_systems.npz (its C, eps, n_occ and E_SCF: the reference's own RHF orbitals at EXTREME convergence), and
H2/STO-3G (dim = 1, its own reference SCF): the AO integrals and dipole matrices, then the reference's run_excited_state_calculation
(tuna_ci.py:2150-2290) with everything it calls -- the AO->MO transformation, calculate_A_matrix / calculate_B_matrix, the eigh of CIS
and the non-symmetric 2 dim eig of TDHF, the transition dipoles, the merge and sort, the printing -- executed from the source text,
never copied; Constants, bohr_to_angstrom, symmetrise and the spacers come from tuna_util.py the same way.  Stored per system: C, eps,
n_occ, E_SCF, dip [3, N, N] (origin: the midpoint of the bond; a transition dipole does not depend on it), and for CIS and TDHF,
all-electron (fc0) and with one frozen orbital (fc1, where o > 1): E_singlet, E_triplet (all states), and of the merged, sorted list
energies, labels (0 = singlet, 1 = triplet), tdm (|mu|) and osc.  Where the reference's TDHF meets an unstable RHF solution (it warns
of complex excitation energies and drops states: N2/STO-3G, whose core-guess RHF solution has negative CIS energies) only the marker
TDHF_fc<n>_unstable and the numbers of roots it kept are stored.  cis_text.json holds what the reference prints for two input lines of
CO/6-31G (one CIS, one TDHF with NSTATES 5), from the excited-state header to the end of the spectrum table, and the .npz the state
vectors those blocks were printed from (text_<n>_X, text_<n>_Y [n_states, o, v], in the merged order).  Only data is written.
"""
from __future__ import annotations

import ast
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from make_golden_mp3 import MP3_SYSTEMS  # noqa: E402
from tuna_amd import guess as guess_mod  # noqa: E402
from tuna_amd import molecule as mol  # noqa: E402

CI_FUNCTIONS = ("transform_ERI_AO_to_MO", "transform_matrix_AO_to_SO", "begin_spatial_orbital_calculation", "calculate_oscillator_strengths",
                "calculate_A_matrix", "calculate_B_matrix", "split_state_vector", "calculate_time_dependent_hartree_fock_states",
                "print_initial_excited_state_information", "calculate_restricted_single_reference_excited_states",
                "calculate_restricted_transition_dipoles", "determine_restricted_excited_state_energy_and_density",
                "print_excited_state_absorption_spectrum", "print_excited_state_contributions", "run_excited_state_calculation")
UTIL_FUNCTIONS = ("bohr_to_angstrom", "symmetrise", "log_spacer", "log_big_spacer")
SYSTEMS = dict(MP3_SYSTEMS, h2_sto3g=(["H", "H"], mol.angstrom_to_bohr(0.74), "STO-3G", 1, False))
TEXT_CASES = [("SPE : C O 1.128 : CIS 6-31G", "co_631g", "CIS", 10), ("SPE : C O 1.128 : TDHF 6-31G : NSTATES 5", "co_631g", "TDHF", 5)]


def load_reference_excited_states():
    """run_excited_state_calculation and what it calls from tuna_ci.py source text, on the helpers of tuna_util.py from source text.
    Returns (namespace, stream, seen): stream collects what log() would print (priority <= 2), seen the intermediate results."""
    stream, seen = [], {}

    def log(message, calculation=None, priority=1, silent=False, end="\n", colour=None):
        if not silent and priority <= 2:
            stream.append(message + end)
    util = {"np": np, "ndarray": np.ndarray, "log": log}
    lines, _ = mg._parseable_lines(os.path.join(mg.REF, "TUNA", "tuna_util.py"))
    found = []
    for node in ast.parse("\n".join(lines)).body:
        if (isinstance(node, ast.FunctionDef) and node.name in UTIL_FUNCTIONS) or (isinstance(node, ast.ClassDef) and node.name == "Constants"):
            if isinstance(node, ast.ClassDef):
                exec(compile(ast.Module([node], []), "tuna_util.py", "exec"), util)
                util["constants"] = util["Constants"]()
            else:
                exec(compile(ast.Module([node], []), "tuna_util.py", "exec"), util)
            found.append(node.name)
    assert sorted(found) == sorted(UTIL_FUNCTIONS + ("Constants",)), found

    def error(msg):
        raise RuntimeError(msg)

    def warning(message, space=1):
        seen.setdefault("warnings", []).append(message)
    base = {"np": np, "ndarray": np.ndarray, "Calculation": object, "Molecule": object, "Output": object, "log": log, "timer": lambda *a, **k: None,
            "error": error, "warning": warning, "constants": util["constants"],
            **{k: util[k] for k in UTIL_FUNCTIONS}}
    from make_golden_ccd import _functions
    ns = _functions(os.path.join(mg.REF, "TUNA", "tuna_ci.py"), CI_FUNCTIONS, dict(base))
    solve, spectrum, contributions, header = (ns[k] for k in ("calculate_restricted_single_reference_excited_states",
                                                              "print_excited_state_absorption_spectrum", "print_excited_state_contributions",
                                                              "print_initial_excited_state_information"))

    def solve_seen(*a, **k):
        r = solve(*a, **k)
        seen["E_singlet"], seen["E_triplet"] = r[0], r[1]
        return r

    def header_seen(*a, **k):
        seen["text_start"] = len(stream)
        return header(*a, **k)

    def contributions_seen(calculation, silent, excitation_energies, excitation_vectors, state_types, n_occ, n_virt, *a, **k):
        seen["vectors"], seen["n_occ"], seen["n_virt"] = excitation_vectors, n_occ, n_virt
        return contributions(calculation, silent, excitation_energies, excitation_vectors, state_types, n_occ, n_virt, *a, **k)

    def spectrum_seen(molecule, excitation_energies, calculation, transition_dipoles, oscillator_strengths, state_types, *a, **k):
        seen.update(energies=excitation_energies, tdm=transition_dipoles, osc=oscillator_strengths, labels=state_types)
        return spectrum(molecule, excitation_energies, calculation, transition_dipoles, oscillator_strengths, state_types, *a, **k)
    ns.update(calculate_restricted_single_reference_excited_states=solve_seen, print_excited_state_absorption_spectrum=spectrum_seen,
              print_excited_state_contributions=contributions_seen, print_initial_excited_state_information=header_seen)
    return ns, stream, seen


def main():
    assert mg.orc.ref_engine() is not None, "run oracle/build_ref.sh first"
    blocks, ortho = mg.load_reference_kernel_bits()
    scf = mg.load_reference_scf()
    ns, stream, seen = load_reference_excited_states()
    z = np.load(os.path.join(mg.GOLD, "mp3_systems.npz"))
    out, texts = {}, []
    for tag, (sym, R, basis, nocc, damp) in SYSTEMS.items():
        atoms, shells, aos = mg.system(sym, R, basis)
        S, T, V, D, Q, E = mg.one_e_and_eri(atoms, aos)
        U = mg.reference_U(shells, blocks)
        Es = mg.eri_to_spherical(U, E)
        dip = np.array([mg.to_spherical(U, d) for d in D])
        if f"{tag}__C" in z.files:
            C, eps, E_SCF = z[f"{tag}__C"], z[f"{tag}__eps"], float(z[f"{tag}__E_SCF"])
            assert int(z[f"{tag}__n_occ"]) == nocc
        else:
            r = mg.run_reference_scf(scf, ortho, atoms, shells, mg.to_spherical(U, S), mg.to_spherical(U, T), mg.to_spherical(U, V), Es, nocc,
                                     "extreme", damp)
            C, eps, E_SCF = r["C"], r["epsilons"], float(r["energy"])
        N = len(eps)
        P = 2.0 * C[:, :nocc] @ C[:, :nocc].T
        d = dict(C=C, eps=eps, n_occ=nocc, E_SCF=E_SCF, dip=dip)
        com = guess_mod.centre_of_mass(atoms) if len(atoms) == 2 else 0.0

        def run(method, nf, n_states=10, root=1):
            calc = types.SimpleNamespace(method=types.SimpleNamespace(name=method, density_functional_method=False, excited_state_method=True),
                                         tamm_dancoff_approximation=False, calculate_no_singlets=False, calculate_no_triplets=False, reference="RHF",
                                         HFX_prop=1.0, root=root, n_states=n_states, excited_state_contribution_threshold=1.0, freeze_core=nf > 0,
                                         do_perturbative_doubles=False, plot_absorbance_spectrum=False, functional=None)
            molecule = types.SimpleNamespace(n_core_orbitals=nf, n_electrons=2 * nocc, n_doubly_occ=nocc, n_doubly_virt=N - nocc, centre_of_mass=com)
            scf_out = types.SimpleNamespace(integrals=types.SimpleNamespace(ERI_AO=Es), molecular_orbitals=C, epsilons=eps, D=dip, P=P, P_alpha=P / 2,
                                            P_beta=P / 2, energy=E_SCF)
            stream.clear(); seen.clear()
            state = ns["run_excited_state_calculation"](molecule, calc, scf_out, None, None, False)
            dim = (nocc - nf) * (N - nocc)
            if seen.get("warnings") or len(seen["E_singlet"]) != dim or len(seen["E_triplet"]) != dim:
                # an unstable reference: the eig of the 2 dim problem has complex or missing roots, which the reference drops with a warning
                assert method == "TDHF", (tag, method, nf, seen.get("warnings"))
                return dict(unstable=1, n_real_singlet=len(seen["E_singlet"]), n_real_triplet=len(seen["E_triplet"]))
            assert len(seen["E_singlet"]) == dim and len(seen["E_triplet"]) == dim, (tag, method, nf, len(seen["E_singlet"]), len(seen["E_triplet"]), dim)
            assert abs(state[0] - (E_SCF + seen["energies"][root - 1])) < 1e-12
            return dict(E_singlet=np.array(seen["E_singlet"]), E_triplet=np.array(seen["E_triplet"]), energies=np.array(seen["energies"]),
                        labels=np.array([0 if s == "singlet" else 1 for s in seen["labels"]], dtype=np.uint8), tdm=np.array(seen["tdm"], dtype=float),
                        osc=np.array(seen["osc"], dtype=float))
        for method in ("CIS", "TDHF"):
            for nf in ((0, 1) if nocc > 1 else (0,)):
                r = run(method, nf)
                d.update({f"{method}_fc{nf}_{k}": val for k, val in r.items()})
                if "unstable" in r:
                    print("CIS", tag, method, f"fc{nf}", "UNSTABLE reference: no TDHF golden", r, flush=True)
                    continue
                print("CIS", tag, method, f"fc{nf}", "dim", len(r["E_singlet"]), "lowest singlet", r["E_singlet"][0], "lowest triplet", r["E_triplet"][0],
                      "sum f", r["osc"].sum(), flush=True)
        for n, (line, system, method, n_states) in enumerate(TEXT_CASES):
            if system != tag:
                continue
            r = run(method, 0, n_states=n_states)
            text = "".join(stream[seen["text_start"]:])
            o, v = seen["n_occ"], seen["n_virt"]
            vec = seen["vectors"][:, :n_states]
            X = vec[:o * v].T.reshape(n_states, o, v)
            Y = vec[o * v:].T.reshape(n_states, o, v) if vec.shape[0] == 2 * o * v else np.zeros_like(X)
            d[f"text_{n}_X"], d[f"text_{n}_Y"] = X, Y
            texts.append(dict(line=line, system=system, method=method, n_states=n_states, prefix=f"{method}_fc0_", vectors=f"text_{n}_", text=text))
        out[tag] = d
    np.savez_compressed(os.path.join(mg.GOLD, "cis_systems.npz"), **{f"{t}__{k}": v for t, d in out.items() for k, v in d.items()})
    with open(os.path.join(mg.GOLD, "cis_text.json"), "w") as f:
        json.dump(texts, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
