#!/usr/bin/env python3
"""Generate tests/golden/ucis_systems.npz and tests/golden/stability_text.json: unrestricted CIS / TDHF and the SCF stability analysis
of the REAL reference (needs oracle/_ref, `bash oracle/build_ref.sh`).

Open shells: the UHF orbitals of tests/golden/ump2_systems.npz (the reference's own UHF cycle at EXTREME convergence) for O2 triplet
in STO-3G and cc-pVDZ, NO/6-31G, OH/cc-pVDZ, Li/6-31G and H/cc-pVDZ.  Per system the AO integrals and dipole matrices, then the
reference's run_excited_state_calculation on its "UHF" branch (tuna_ci.py:2215-2290) with everything it calls -- the spin-blocked
transformation, calculate_A_matrix / calculate_B_matrix, the eigh of CIS and the non-symmetric eig of TDHF, the transition dipoles, the
printing -- and determine_self_consistent_field_stability (:1049-1106), executed from the source text, never copied.  Stored per
system: C_alpha, C_beta, eps_alpha, eps_beta, n_alpha, n_beta, E_UHF, dip [3, N, N], and per variant fc<k> (k frozen spin orbitals, k / 2
of either spin): CIS_fc<k>_energies / tdm (|mu|) / osc, the same for TDHF -- or, where the reference's TDHF warns of complex energies or
drops roots, or its Hessian is not positive definite (UNSTABLE_BELOW, ZERO_MODE_BELOW below), only TDHF_fc<k>_unstable or
TDHF_fc<k>_marginal -- and stab_fc<k>_lowest, the lowest eigenvalue of the reference's Hessian of order 2 dim.

Two conditions tie the reference's energy-sorted spin orbitals to the library's windows and are asserted here: the lowest n_occ of the
combined sorted spin-orbital energies are the n_alpha lowest alpha plus the n_beta lowest beta orbitals, and the frozen ones split evenly
between the spins.  At least three open-shell systems must have a stable TDHF golden.

Closed shells: for the molecules of tests/golden/cis_systems.npz (its orbitals) and H2/STO-3G at 0.74 and 2.0 angstrom (the reference's
own RHF cycle), rstab__<tag>__singlet / triplet: the lowest eigenvalues of the reference's singlet and triplet Hessians.

stability_text.json: what the reference prints for the stability block of three input lines, and its unrestricted contribution and
spectrum blocks for O2/STO-3G (UCIS) and Li/6-31G (UTDHF), 5 states each; the .npz holds the vectors those blocks were printed from in the library's
index order (text_<n>_X, text_<n>_Y [n_states, dim]: alpha block, then beta block).  Only data is written.
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
from make_golden_ccd import _functions  # noqa: E402
from make_golden_cis import SYSTEMS as CIS_SYSTEMS  # noqa: E402
from make_golden_cis import UTIL_FUNCTIONS  # noqa: E402
from make_golden_ump2 import UMP2_SYSTEMS  # noqa: E402
from tuna_amd import guess as guess_mod  # noqa: E402
from tuna_amd import molecule as mol  # noqa: E402

CI_FUNCTIONS = ("spin_block_molecular_orbitals", "transform_ERI_AO_to_SO", "antisymmetrise_integrals", "transform_ERI_AO_to_MO",
                "transform_matrix_AO_to_SO", "transform_P_SO_to_AO", "begin_spin_orbital_calculation", "begin_spatial_orbital_calculation",
                "calculate_oscillator_strengths", "calculate_A_matrix", "calculate_B_matrix", "build_orbital_hessian",
                "perform_restricted_stability_analysis", "perform_unrestricted_stability_analysis", "determine_self_consistent_field_stability",
                "split_state_vector", "calculate_time_dependent_hartree_fock_states", "print_initial_excited_state_information",
                "calculate_unrestricted_single_reference_excited_states", "calculate_unrestricted_transition_dipoles",
                "determine_unrestricted_excited_state_energy_and_density", "print_excited_state_absorption_spectrum",
                "print_excited_state_contributions", "run_excited_state_calculation")
# tag -> frozen spin orbitals of its variants
OPEN_SHELLS = {"o2_triplet_sto3g": (0,), "o2_triplet_ccpvdz": (0, 4), "no_doublet_631g": (0,), "oh_doublet_ccpvdz": (0,), "li_doublet_631g": (0,),
               "h_ccpvdz": (0,)}
H2_STRETCHED = dict(h2_sto3g=0.74, h2_sto3g_2p0=2.0)
TEXT_EXCITED = [("o2_triplet_sto3g", "UCIS", 5), ("li_doublet_631g", "UTDHF", 5)]
# The TDHF of a system is a golden only where the symmetric reduction the library solves exists: A + B and A - B both positive definite,
# that is the reference's lowest Hessian eigenvalue above zero.  At or below the reference's own instability threshold (tuna_util.py:
# ORB_HESS_EIG_THRESH) the system is marked unstable, whatever the reference's non-symmetric eig returned (for O2/STO-3G, a saddle point
# with lowest eigenvalue -0.263, it returns 30 real roots and no warning); between that and 1e-6 the Hessian has a zero mode (the
# rotation of the singly occupied pi orbital of NO and OH) and the outcome of either program is decided by rounding: marked marginal.
UNSTABLE_BELOW = -1e-5
ZERO_MODE_BELOW = 1e-6
TEXT_STABILITY = [("SPE : H H 2.0 : HF STO-3G : STAB", "h2_sto3g_2p0"), ("SPE : C O 1.128 : HF 6-31G : STAB", "co_631g"),
                  ("SPE : O O 1.2075 : UHF STO-3G : ML 3 STAB", "o2_triplet_sto3g")]


def load_reference():
    """The functions of CI_FUNCTIONS from tuna_ci.py source text on the helpers of tuna_util.py from source text.  Returns (namespace,
    stream, seen): stream collects what log() would print (priority <= 2), seen the intermediate results."""
    stream, seen = [], {}

    def log(message, calculation=None, priority=1, silent=False, end="\n", colour=None):
        if not silent and priority <= 2:
            stream.append(message + end)
    util = {"np": np, "ndarray": np.ndarray, "log": log}
    lines, _ = mg._parseable_lines(os.path.join(mg.REF, "TUNA", "tuna_util.py"))
    found = []
    for node in ast.parse("\n".join(lines)).body:
        if (isinstance(node, ast.FunctionDef) and node.name in UTIL_FUNCTIONS) or (isinstance(node, ast.ClassDef) and node.name == "Constants"):
            exec(compile(ast.Module([node], []), "tuna_util.py", "exec"), util)
            if isinstance(node, ast.ClassDef):
                util["constants"] = util["Constants"]()
            found.append(node.name)
    assert sorted(found) == sorted(UTIL_FUNCTIONS + ("Constants",)), found

    def error(msg):
        raise RuntimeError(msg)

    def warning(message, space=1):
        seen.setdefault("warnings", []).append(message)
    base = {"np": np, "ndarray": np.ndarray, "Calculation": object, "Molecule": object, "Output": object, "log": log, "timer": lambda *a, **k: None,
            "error": error, "warning": warning, "constants": util["constants"], **{k: util[k] for k in UTIL_FUNCTIONS}}
    ns = _functions(os.path.join(mg.REF, "TUNA", "tuna_ci.py"), CI_FUNCTIONS, dict(base))
    begin, hessian, contributions, spectrum = (ns[k] for k in ("begin_spin_orbital_calculation", "build_orbital_hessian", "print_excited_state_contributions",
                                                               "print_excited_state_absorption_spectrum"))

    def begin_seen(*a, **k):
        r = begin(*a, **k)
        seen["spin_orbital_labels"] = list(r[7])
        return r

    def hessian_seen(*a, **k):
        H = hessian(*a, **k)
        seen.setdefault("hessian_lowest", []).append(float(np.linalg.eigh(H)[0][0]))      # (the reference's own call, tuna_ci.py:962, :1024)
        return H

    def contributions_seen(calculation, silent, excitation_energies, excitation_vectors, *a, **k):
        seen["text_start"] = len(stream)
        seen["vectors"] = excitation_vectors
        return contributions(calculation, silent, excitation_energies, excitation_vectors, *a, **k)

    def spectrum_seen(molecule, excitation_energies, calculation, transition_dipoles, oscillator_strengths, state_types, *a, **k):
        seen.update(energies=excitation_energies, tdm=transition_dipoles, osc=oscillator_strengths)
        return spectrum(molecule, excitation_energies, calculation, transition_dipoles, oscillator_strengths, state_types, *a, **k)
    ns.update(begin_spin_orbital_calculation=begin_seen, build_orbital_hessian=hessian_seen, print_excited_state_contributions=contributions_seen,
              print_excited_state_absorption_spectrum=spectrum_seen)
    return ns, stream, seen


def stability_block(stream):
    """The printed block from the spacer above "Stability Analysis" to the closing spacer"""
    k = next(n for n, s in enumerate(stream) if "Stability Analysis" in s)
    return "".join(stream[k - 1:])


def library_order(labels, n_occ_spin, n_virt_spin, windows, N):
    """Rows of the reference's [n_occ_spin * n_virt_spin] excitation space (energy-sorted spin orbitals, o = [n_frozen, n_occ)) that the
    library's compound index addresses, in its order: alpha block (ia) = i v_a + a, then beta.  windows = ((n_a, nf_a), (n_b, nf_b))."""
    pos = {lab: k for k, lab in enumerate(labels)}
    n_occ_total = sum(n for n, _ in windows)
    n_frozen_total = sum(nf for _, nf in windows)
    rows = []
    for spin, (n, nf) in zip("ab", windows):
        for i in range(nf, n):
            for a in range(n, N):
                I, A = pos[f"{i + 1}{spin}"], pos[f"{a + 1}{spin}"]
                assert n_frozen_total <= I < n_occ_total <= A, (spin, i, a, I, A)
                rows.append((I - n_frozen_total) * n_virt_spin + (A - n_occ_total))
    assert len(set(rows)) == len(rows)
    return np.array(rows, dtype=int)


def main():
    assert mg.orc.ref_engine() is not None, "run oracle/build_ref.sh first"
    blocks, ortho = mg.load_reference_kernel_bits()
    scf = mg.load_reference_scf()
    ns, stream, seen = load_reference()
    zu = np.load(os.path.join(mg.GOLD, "ump2_systems.npz"))
    zc = np.load(os.path.join(mg.GOLD, "cis_systems.npz"))
    out, texts, n_text, stable_tdhf = {}, [], 0, 0

    def method_ns(name):
        return types.SimpleNamespace(name=name, density_functional_method=False, excited_state_method=True, unrestricted_available=True)

    def calculation(name, reference, n_frozen, n_states=10, root=1):
        return types.SimpleNamespace(method=method_ns(name), tamm_dancoff_approximation=False, calculate_no_singlets=False, calculate_no_triplets=False,
                                     reference=reference, HFX_prop=1.0, root=root, n_states=n_states, excited_state_contribution_threshold=1.0,
                                     freeze_core=n_frozen > 0, do_perturbative_doubles=False, plot_absorbance_spectrum=False, functional=None)

    def integrals(sym, R, basis):
        atoms, shells, aos = mg.system(sym, R, basis)
        S, T, V, D, Q, E = mg.one_e_and_eri(atoms, aos)
        U = mg.reference_U(shells, blocks)
        return atoms, shells, U, (S, T, V), mg.eri_to_spherical(U, E), np.array([mg.to_spherical(U, d) for d in D])

    # ---- open shells
    for tag, variants in OPEN_SHELLS.items():
        sym, R, basis, na, nb, _ = UMP2_SYSTEMS[tag]
        atoms, shells, U, _, Es, dip = integrals(sym, R, basis)
        Ca, Cb, ea, eb, E_UHF = (zu[f"{tag}__{k}"] for k in ("C_alpha", "C_beta", "eps_alpha", "eps_beta", "E_UHF"))
        assert int(zu[f"{tag}__n_alpha"]) == na and int(zu[f"{tag}__n_beta"]) == nb
        N = len(ea)
        Pa, Pb = Ca[:, :na] @ Ca[:, :na].T, Cb[:, :nb] @ Cb[:, :nb].T
        com = guess_mod.centre_of_mass(atoms) if len(atoms) == 2 else 0.0
        d = dict(C_alpha=Ca, C_beta=Cb, eps_alpha=ea, eps_beta=eb, n_alpha=na, n_beta=nb, E_UHF=float(E_UHF), dip=dip)
        scf_out = types.SimpleNamespace(integrals=types.SimpleNamespace(ERI_AO=Es), molecular_orbitals_alpha=Ca, molecular_orbitals_beta=Cb,
                                        epsilons_alpha=ea, epsilons_beta=eb, epsilons_combined=np.append(ea, eb), D=dip, P=Pa + Pb, P_alpha=Pa, P_beta=Pb,
                                        energy=float(E_UHF))
        # the reference's occupied and frozen spin orbitals against the windows of either spin
        order = np.argsort(np.append(ea, eb))
        spins = np.array(["a"] * N + ["b"] * N)[order]
        assert int(np.sum(spins[:na + nb] == "a")) == na, (tag, "the lowest n_occ spin orbitals are not n_alpha alpha + n_beta beta")
        for k in variants:
            assert k % 2 == 0 and int(np.sum(spins[:k] == "a")) == k // 2, (tag, k, "the frozen spin orbitals do not split evenly")

        def molecule_ns(k):
            return types.SimpleNamespace(n_core_spin_orbitals=k, n_core_orbitals=k // 2, n_electrons=na + nb, n_occ=na + nb, n_virt=2 * N - na - nb,
                                         centre_of_mass=com)

        def run(method, k, n_states=10):
            stream.clear(); seen.clear()
            calc = calculation(method, "UHF", k, n_states)
            state = ns["run_excited_state_calculation"](molecule_ns(k), calc, scf_out, None, None, False)
            dim = (na - k // 2) * (N - na) + (nb - k // 2) * (N - nb)
            if seen.get("warnings") or len(seen["energies"]) != dim:
                assert "TDHF" in method, (tag, method, k, seen.get("warnings"))
                return dict(unstable=1, n_real=len(seen["energies"]))
            assert abs(state[0] - (float(E_UHF) + seen["energies"][0])) < 1e-12
            return dict(energies=np.array(seen["energies"]), tdm=np.array(seen["tdm"], dtype=float), osc=np.array(seen["osc"], dtype=float))
        for k in variants:
            stream.clear(); seen.clear()
            ns["determine_self_consistent_field_stability"](molecule_ns(k), calculation("UHF", "UHF", k), Es, scf_out, None, None, False)
            assert len(seen["hessian_lowest"]) == 1
            lowest = d[f"stab_fc{k}_lowest"] = seen["hessian_lowest"][0]
            print("STAB", tag, f"fc{k}", lowest, flush=True)
            if k == 0:
                for line, system in TEXT_STABILITY:
                    if system == tag:
                        texts.append(dict(kind="stability", line=line, system=tag, reference="UHF", lowest=[lowest], text=stability_block(stream)))
            for method in ("UCIS", "UTDHF"):
                r = run(method, k)
                if method == "UTDHF" and lowest <= UNSTABLE_BELOW:
                    r = dict(unstable=1, n_real=r.get("n_real", len(r.get("energies", ()))))
                elif method == "UTDHF" and lowest < ZERO_MODE_BELOW:
                    r = dict(marginal=1, n_real=r.get("n_real", len(r.get("energies", ()))))
                d.update({f"{method[1:]}_fc{k}_{key}": val for key, val in r.items()})
                if "energies" not in r:
                    print("UCIS", tag, method, f"fc{k}", "no TDHF golden", r, flush=True)
                else:
                    stable_tdhf += method == "UTDHF" and k == 0 and na != nb
                    print("UCIS", tag, method, f"fc{k}", "dim", len(r["energies"]), "lowest", r["energies"][0], "sum f", r["osc"].sum(), flush=True)
        for system, method, n_states in TEXT_EXCITED:
            if system != tag:
                continue
            r = run(method, 0, n_states)
            if "unstable" in r or d.get(f"{method[1:]}_fc0_unstable") or d.get(f"{method[1:]}_fc0_marginal"):
                continue
            text = "".join(stream[seen["text_start"]:])
            n_occ_spin, n_virt_spin = na + nb, 2 * N - na - nb
            rows = library_order(seen["spin_orbital_labels"], n_occ_spin, n_virt_spin, ((na, 0), (nb, 0)), N)
            vec = seen["vectors"][:, :n_states]
            full = n_occ_spin * n_virt_spin
            X = vec[:full][rows].T
            Y = vec[full:][rows].T if vec.shape[0] == 2 * full else np.zeros_like(X)
            assert abs(np.sum(vec[:full] ** 2) - np.sum(X ** 2)) < 1e-12          # nothing outside the spin-conserving rows
            d[f"text_{n_text}_X"], d[f"text_{n_text}_Y"] = X, Y
            texts.append(dict(kind="excited", system=tag, method=method[1:], n_states=n_states, prefix=f"{method[1:]}_fc0_", vectors=f"text_{n_text}_",
                              labels=seen["spin_orbital_labels"], text=text))
            n_text += 1
        out[tag] = d
    assert stable_tdhf >= 3, f"only {stable_tdhf} open-shell systems have a stable TDHF golden: add small systems until three do"
    # ---- closed shells: the restricted stability numbers
    rstab = {}
    closed = {tag: (CIS_SYSTEMS[tag], None) for tag in CIS_SYSTEMS if tag != "h2_sto3g"}
    closed.update({tag: ((["H", "H"], mol.angstrom_to_bohr(R), "STO-3G", 1, False), R) for tag, R in H2_STRETCHED.items()})
    for tag, ((sym, R, basis, nocc, damp), _) in closed.items():
        atoms, shells, U, (S, T, V), Es, dip = integrals(sym, R, basis)
        if f"{tag}__C" in zc.files:
            C, eps, E_SCF = zc[f"{tag}__C"], zc[f"{tag}__eps"], float(zc[f"{tag}__E_SCF"])
        else:
            r = mg.run_reference_scf(scf, ortho, atoms, shells, mg.to_spherical(U, S), mg.to_spherical(U, T), mg.to_spherical(U, V), Es, nocc, "extreme", damp)
            C, eps, E_SCF = r["C"], r["epsilons"], float(r["energy"])
            rstab[f"{tag}__C"], rstab[f"{tag}__eps"], rstab[f"{tag}__E_SCF"] = C, eps, E_SCF
        N = len(eps)
        molecule = types.SimpleNamespace(n_core_orbitals=0, n_electrons=2 * nocc, n_doubly_occ=nocc, n_doubly_virt=N - nocc)
        scf_out = types.SimpleNamespace(integrals=types.SimpleNamespace(ERI_AO=Es), molecular_orbitals=C, epsilons=eps, energy=E_SCF)
        # the restricted transformation reads the AO tensor as ERI_AO[m, k, n, l] = (mn|kl) (tuna_ci.py:227-229).  Checked where the
        # reference's own CIS is stored: the lowest eigenvalue of its singlet A from this tensor is the golden's lowest CIS singlet
        Ei = np.ascontiguousarray(Es.transpose(0, 2, 1, 3))
        calc = calculation("HF", "RHF", 0)
        if f"{tag}__CIS_fc0_E_singlet" in zc.files:
            g = ns["transform_ERI_AO_to_MO"](Ei, C, calc, True)
            A_singlet = ns["calculate_A_matrix"](calc, g, eps, slice(0, nocc), slice(nocc, None), None, "singlet")
            assert abs(np.linalg.eigvalsh(A_singlet)[0] - zc[f"{tag}__CIS_fc0_E_singlet"][0]) < 1e-10, tag
        stream.clear(); seen.clear()
        ns["determine_self_consistent_field_stability"](molecule, calc, Ei, scf_out, None, None, False)
        assert len(seen["hessian_lowest"]) == 2
        rstab[f"{tag}__singlet"], rstab[f"{tag}__triplet"] = seen["hessian_lowest"]
        print("RSTAB", tag, seen["hessian_lowest"], flush=True)
        for line, system in TEXT_STABILITY:
            if system == tag:
                texts.append(dict(kind="stability", line=line, system=tag, reference="RHF", lowest=list(seen["hessian_lowest"]), text=stability_block(stream)))
    data = {f"{t}__{k}": v for t, d in out.items() for k, v in d.items()}
    data.update({f"rstab__{k}": v for k, v in rstab.items()})
    np.savez_compressed(os.path.join(mg.GOLD, "ucis_systems.npz"), **data)
    with open(os.path.join(mg.GOLD, "stability_text.json"), "w") as f:
        json.dump(texts, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
