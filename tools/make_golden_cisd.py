#!/usr/bin/env python3
"""Generate tests/golden/cisd_systems.npz and tests/golden/cisd_text.json: the perturbative doubles correction CIS(D) of the REAL
reference (needs oracle/_ref, `bash oracle/build_ref.sh`).

Per system of tests/golden/cis_systems.npz (its C, eps, n_occ and E_SCF are read from there and not stored again), all-electron (fc0)
and with one frozen orbital (fc1, where o > 1): the reference's run_excited_state_calculation with do_perturbative_doubles, executed
from the source text as tools/make_golden_cis.py does, which hands run_perturbative_doubles (tuna_ci.py:2090-2139) its MO tensor, its
merged and sorted states and their vectors.  From these, for the lowest four singlets and the lowest four triplets of CIS (fewer where
dim is smaller) -- and for co_631g of TDHF as well, with b = X + Y (:2117-2119) -- calculate_restricted_doubles_correction
(:1874-1982) is called state by state.  Stored per system, method and frozen count, <method>_fc<n>_: b [n, o, v], omega [n], triplet
[n] (0 = singlet, 1 = triplet), E_D [n], min_denominator [n] = min over ijab of |e_i + e_j - e_a - e_b + omega|, and index [n], the
state's place in the merged list.  A state whose min_denominator is not above 0.1 Eh is dropped (a near-resonant denominator would
loosen every tolerance of the tests); at least three states per multiplicity must remain wherever dim >= 4.  cisd_text.json holds
what the reference prints for the (D) section of two input lines of CO/6-31G (one CIS, one TDHF), at priorities <= 2, with the root's
b, omega, flag, E_D and E_SCF.  Only data is written."""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
import make_golden_cis as mgc  # noqa: E402
from tuna_amd import guess as guess_mod  # noqa: E402

CISD_FUNCTIONS = ("build_doubles_epsilons_tensor", "build_MP2_t_amplitudes", "calculate_restricted_doubles_correction", "run_perturbative_doubles")
N_PER_MULTIPLICITY = 4
MIN_DENOMINATOR = 0.1             # Eh
TDHF_SYSTEMS = ("co_631g",)
TEXT_CASES = [("SPE : C O 1.128 : CIS 6-31G : (D)", "co_631g", "CIS"), ("SPE : C O 1.128 : TDHF 6-31G : (D)", "co_631g", "TDHF")]


def load_reference():
    """make_golden_cis's namespace with the functions of the (D) step added; run_perturbative_doubles records what it is handed."""
    mgc.CI_FUNCTIONS = tuple(mgc.CI_FUNCTIONS) + CISD_FUNCTIONS
    ns, stream, seen = mgc.load_reference_excited_states()
    doubles = ns["run_perturbative_doubles"]

    def doubles_seen(state, n_occ, n_virt, excitation_vectors, g, epsilons, o, v, state_types, state_of_interest, calculation, silent):
        seen.update(pd_text_start=len(stream), pd_vectors=excitation_vectors, pd_g=g, pd_eps=epsilons, pd_o=o, pd_v=v, pd_types=state_types,
                    pd_n_occ=n_occ, pd_n_virt=n_virt, pd_before=state_of_interest)
        r = doubles(state, n_occ, n_virt, excitation_vectors, g, epsilons, o, v, state_types, state_of_interest, calculation, silent)
        seen["pd_after"] = r
        return r
    ns["run_perturbative_doubles"] = doubles_seen
    return ns, stream, seen


def main():
    assert mg.orc.ref_engine() is not None, "run oracle/build_ref.sh first"
    blocks, _ = mg.load_reference_kernel_bits()
    ns, stream, seen = load_reference()
    z = np.load(os.path.join(mg.GOLD, "cis_systems.npz"))
    out, texts = {}, []
    for tag, (sym, R, basis, nocc, damp) in mgc.SYSTEMS.items():
        atoms, shells, aos = mg.system(sym, R, basis)
        S, T, V, D, Q, E = mg.one_e_and_eri(atoms, aos)
        U = mg.reference_U(shells, blocks)
        Es = mg.eri_to_spherical(U, E)
        C, eps, E_SCF, dip = z[f"{tag}__C"], z[f"{tag}__eps"], float(z[f"{tag}__E_SCF"]), z[f"{tag}__dip"]
        assert int(z[f"{tag}__n_occ"]) == nocc
        N = len(eps)
        P = 2.0 * C[:, :nocc] @ C[:, :nocc].T
        com = guess_mod.centre_of_mass(atoms) if len(atoms) == 2 else 0.0

        def run(method, nf):
            """One reference run with the (D) step on ROOT 1; returns (calc, what the run left in seen, the printed (D) section)."""
            calc = types.SimpleNamespace(method=types.SimpleNamespace(name=method, density_functional_method=False, excited_state_method=True),
                                         tamm_dancoff_approximation=False, calculate_no_singlets=False, calculate_no_triplets=False, reference="RHF",
                                         HFX_prop=1.0, root=1, n_states=10, excited_state_contribution_threshold=1.0, freeze_core=nf > 0,
                                         do_perturbative_doubles=True, plot_absorbance_spectrum=False, functional=None, MPC_requested=False,
                                         DFT_calculation=False, MPC_prop=1.0)
            molecule = types.SimpleNamespace(n_core_orbitals=nf, n_electrons=2 * nocc, n_doubly_occ=nocc, n_doubly_virt=N - nocc, centre_of_mass=com)
            scf_out = types.SimpleNamespace(integrals=types.SimpleNamespace(ERI_AO=Es), molecular_orbitals=C, epsilons=eps, D=dip, P=P, P_alpha=P / 2,
                                            P_beta=P / 2, energy=E_SCF)
            stream.clear(); seen.clear()
            state = ns["run_excited_state_calculation"](molecule, calc, scf_out, None, None, False)
            assert not seen.get("warnings"), (tag, method, nf, seen.get("warnings"))
            text = "".join(stream[seen["pd_text_start"]:])
            assert abs(state[0] - seen["pd_after"][0]) == 0 and abs(state[1] - (seen["energies"][0] + (state[0] - seen["pd_before"][0]))) < 1e-14
            return calc, dict(seen), text, state

        def states(calc, s, wanted):
            """b, omega, flag, E_D and min |D + omega| of the merged states `wanted`, by the reference's own function"""
            o, v, n_occ, n_virt = s["pd_o"], s["pd_v"], s["pd_n_occ"], s["pd_n_virt"]
            e = np.asarray(s["pd_eps"])
            Dijab = e[o][:, None, None, None] + e[o][None, :, None, None] - e[v][None, None, :, None] - e[v][None, None, None, :]
            rows = []
            for n in wanted:
                X, Y = ns["split_state_vector"](s["pd_vectors"][:, n], n_occ, n_virt)
                b, w, kind = X + Y, float(s["energies"][n]), str(s["pd_types"][n])
                E_D = ns["calculate_restricted_doubles_correction"](w, s["pd_eps"], n, s["pd_g"].transpose(0, 2, 1, 3), o, v, b, kind, calc, True)
                rows.append((np.array(b, dtype=float).reshape(n_occ, n_virt), w, int(kind == "triplet"), float(E_D), float(np.abs(Dijab + w).min()), n))
            return rows

        d = {}
        for method in ("CIS",) + (("TDHF",) if tag in TDHF_SYSTEMS else ()):
            for nf in ((0, 1) if nocc > 1 else (0,)):
                calc, s, text, state = run(method, nf)
                labels, dim = np.asarray(s["labels"]), (nocc - nf) * (N - nocc)
                kept = []
                for kind in ("singlet", "triplet"):
                    mine = [int(n) for n in np.flatnonzero(labels == kind)]
                    good = [r for r in states(calc, s, mine[:N_PER_MULTIPLICITY]) if r[4] > MIN_DENOMINATOR]
                    more = N_PER_MULTIPLICITY
                    while dim >= 4 and len(good) < 3 and more < len(mine):      # (never needed so far: the lowest states are far from resonance)
                        good += [r for r in states(calc, s, mine[more:more + 1]) if r[4] > MIN_DENOMINATOR]
                        more += 1
                    assert len(good) >= min(3, dim) or dim < 4, (tag, method, nf, kind, len(good))
                    kept += good
                kept.sort(key=lambda r: r[5])
                assert all(r[4] > MIN_DENOMINATOR for r in kept) and kept
                pre = f"{method}_fc{nf}_"
                d[pre + "b"] = np.array([r[0] for r in kept])
                d[pre + "omega"] = np.array([r[1] for r in kept])
                d[pre + "triplet"] = np.array([r[2] for r in kept], dtype=np.uint8)
                d[pre + "E_D"] = np.array([r[3] for r in kept])
                d[pre + "min_denominator"] = np.array([r[4] for r in kept])
                d[pre + "index"] = np.array([r[5] for r in kept], dtype=np.int32)
                root = [r for r in kept if r[5] == 0]
                assert root and abs((state[1] - s["energies"][0]) - root[0][3]) < 1e-15       # the run's own (D) step is the same number
                print("CISD", tag, method, f"fc{nf}", "states", len(kept), "E_D", d[pre + "E_D"], "min |D + w|", d[pre + "min_denominator"].min(), flush=True)
                for line, system, m in TEXT_CASES:
                    if system == tag and m == method and nf == 0:
                        texts.append(dict(line=line, system=system, method=method, prefix=pre, E_SCF=E_SCF, omega=root[0][1], triplet=root[0][2],
                                          E_D=root[0][3], text=text))
        out[tag] = d
    np.savez_compressed(os.path.join(mg.GOLD, "cisd_systems.npz"), **{f"{t}__{k}": v for t, d in out.items() for k, v in d.items()})
    with open(os.path.join(mg.GOLD, "cisd_text.json"), "w") as f:
        json.dump(texts, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
