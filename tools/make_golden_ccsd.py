#!/usr/bin/env python3
"""Generate tests/golden/ccsd_systems.npz: restricted LCCSD, QCISD and CCSD of the REAL reference (needs oracle/_ref, `bash oracle/build_ref.sh`).

The construction of make_golden_ccd.py with the singles switched on: per system of tests/golden/mp3_systems.npz (its C, eps and n_occ)
the AO integrals, the reference's AO->MO transformation, then the reference's calculate_coupled_cluster_energy (tuna_cc.py:2950-3175)
with the functions it calls -- the LCCSD, QCISD and CCSD amplitude updates, the energy expression, the convergence test, DIIS and
damping -- executed from the source text, never copied.  The guess is t2 = (ia|jb) / D and t1 = 0 (tuna_cc.py:3267 with a diagonal Fock
matrix), F = diag(eps).  Settings as in ccd_systems.npz: energy convergence 1e-11, amplitude convergence 1e-10, DIIS with 6 vectors, no
damping, at most 100 steps.  Stored per system and method, all-electron (fc0) and with one frozen orbital (fc1): E_corr, n_iter, the
energy of every step (energies), ||t2 - t2_old||_2 and ||t1 - t1_old||_2 of every step (dt2_norms, dt1_norms), the guess energy E_MP2,
the three parts of the energy (E_singles, E_connected, E_disconnected), t1_norm and the final t1 [o][v].  n2_ccpvdz also has a NODIIS
run (nodiis_*) and a CORRDAMP 0.3 run (damp03_*), all-electron.  A system with a run the reference does not converge within 100 steps
is left out (n2_sto3g, as in the CCD goldens).  Only data is written.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from make_golden_ccd import _functions  # noqa: E402
from make_golden_mp3 import MP3_SYSTEMS  # noqa: E402

CC_FUNCTIONS = ("calculate_restricted_coupled_cluster_energy", "coupled_cluster_initial_print", "permute", "is_coupled_cluster_converged",
                "apply_damping", "update_DIIS", "apply_DIIS", "run_restricted_LCCD_iteration", "run_restricted_CCD_iteration",
                "run_restricted_LCCSD_iteration", "run_restricted_QCISD_iteration", "run_restricted_CCSD_iteration",
                "calculate_coupled_cluster_energy")
METHODS = ("LCCSD", "QCISD", "CCSD")
REQUIRED = ("n2_ccpvdz", "n2_ccpvtz", "hf_ccpvdz", "ne_ccpvdz")


def load_reference_cc():
    """calculate_coupled_cluster_energy and what it calls from tuna_cc.py source text, with the tuna_mp / tuna_ci helpers they use.
    Returns (run, trace, ci, mp): trace collects per step the energy and its parts, ||dt2||_2 and ||dt1||_2, and the last t1."""
    stubs = mg._stub_modules()["tuna_util"]
    base = {"np": np, "ndarray": np.ndarray, "Calculation": object, "Method": object, "Output": object, "Integrals": object, "Molecule": object,
            "log": stubs.log, "log_spacer": stubs.log_spacer, "timer": stubs.timer, "error": stubs.error}
    ci = types.SimpleNamespace(**{k: v for k, v in _functions(os.path.join(mg.REF, "TUNA", "tuna_ci.py"),
                                                              ("build_doubles_epsilons_tensor", "build_singles_epsilons_tensor",
                                                               "build_MP2_t_amplitudes"), dict(base)).items() if callable(v)})
    mp = types.SimpleNamespace(**{k: v for k, v in _functions(os.path.join(mg.REF, "TUNA", "tuna_mp.py"), ("calculate_restricted_MP2_energy",),
                                                              dict(base)).items() if callable(v)})
    ns = _functions(os.path.join(mg.REF, "TUNA", "tuna_cc.py"), CC_FUNCTIONS, dict(base, ci=ci, mp=mp))
    trace = {"E": [], "parts": [], "dt2": [], "dt1": [], "t1": None}
    energy, converged = ns["calculate_restricted_coupled_cluster_energy"], ns["is_coupled_cluster_converged"]

    def energy_traced(*a, **k):
        r = energy(*a, **k)
        trace["E"].append(float(r[0]))
        trace["parts"].append([float(x) for x in r[1:4]])
        return r

    def converged_traced(delta_E, t, t_old, calculation):
        trace["dt2"].append(float(np.linalg.norm(t[1] - t_old[1])))
        trace["dt1"].append(float(np.linalg.norm(t[0] - t_old[0])))
        trace["t1"] = np.array(t[0], dtype=float)
        return converged(delta_E, t, t_old, calculation)
    ns["calculate_restricted_coupled_cluster_energy"], ns["is_coupled_cluster_converged"] = energy_traced, converged_traced
    return ns["calculate_coupled_cluster_energy"], trace, ci, mp


def main():
    assert mg.orc.ref_engine() is not None, "run oracle/build_ref.sh first"
    blocks, _ = mg.load_reference_kernel_bits()
    ao_to_mo, _ = mg.load_reference_ao_to_mo()
    run_cc, trace, ci, mp = load_reference_cc()
    z = np.load(os.path.join(mg.GOLD, "mp3_systems.npz"))
    out, left_out = {}, []
    for tag, (sym, R, basis, nocc, _) in MP3_SYSTEMS.items():
        C, eps = z[f"{tag}__C"], z[f"{tag}__eps"]
        assert int(z[f"{tag}__n_occ"]) == nocc
        atoms, shells, aos = mg.system(sym, R, basis)
        E = mg.one_e_and_eri(atoms, aos)[5]
        Es = mg.eri_to_spherical(mg.reference_U(shells, blocks), E)
        N = len(eps)
        g = ao_to_mo(Es, C, None, True).swapaxes(1, 2)           # tuna_cc.py:3229: <pq|rs> = (pr|qs)

        def run(method, nf, diis=True, damping=0.0):
            o, v = slice(nf, nocc), slice(nocc, N)
            e_ijab = ci.build_doubles_epsilons_tensor(eps, eps, o, o, v, v)
            e_ia = ci.build_singles_epsilons_tensor(eps, o, v)
            t_ijab = ci.build_MP2_t_amplitudes(g[o, o, v, v], e_ijab)          # tuna_cc.py:3268
            t_ia = np.zeros_like(e_ia)
            calc = types.SimpleNamespace(energy_convergence=1e-11, amp_conv=1e-10, correlated_max_iter=100, DIIS=diis, max_DIIS_matrices=6,
                                         correlated_damping_parameter=damping, reference="RHF")
            for k in ("E", "parts", "dt2", "dt1"):
                trace[k].clear()
            trace["t1"] = None
            E_MP2 = float(mp.calculate_restricted_MP2_energy(t_ijab, g[o, o, v, v]))
            try:
                E_CC, _ = run_cc(g, o, v, (t_ia, t_ijab, None, None), (e_ia, e_ijab, None, None), np.diag(eps), types.SimpleNamespace(name=method),
                                 calc, True, None, None)
            except RuntimeError as e:                           # the reference's error(): not converged in 100 steps
                print("  left out:", tag, method, nf, diis, damping, e, flush=True)
                return None
            parts = trace["parts"][-1]
            return dict(E_corr=float(E_CC), n_iter=len(trace["E"]), energies=np.array(trace["E"]), dt2_norms=np.array(trace["dt2"]),
                        dt1_norms=np.array(trace["dt1"]), E_MP2=E_MP2, E_singles=parts[0], E_connected=parts[1], E_disconnected=parts[2],
                        t1_norm=float(np.linalg.norm(trace["t1"])), t1=trace["t1"].copy())
        d, ok = {}, True
        for method in METHODS:
            if not ok:
                break
            variants = [(f"{method}_fc0_", dict(nf=0)), (f"{method}_fc1_", dict(nf=1))]
            if tag == "n2_ccpvdz":
                variants += [(f"{method}_nodiis_", dict(nf=0, diis=False)), (f"{method}_damp03_", dict(nf=0, damping=0.3))]
            for pre, kw in variants:
                r = run(method, **kw)
                if r is None:
                    ok = False
                    break
                d.update({pre + k: val for k, val in r.items()})
                print("CC", tag, pre, "E_corr", r["E_corr"], "steps", r["n_iter"], "last dE", r["energies"][-1] - r["energies"][-2], "last |dt2|",
                      r["dt2_norms"][-1], "|t1|", r["t1_norm"], flush=True)
        if ok:
            out[tag] = d
        else:
            left_out.append(tag)
    assert all(t in out for t in REQUIRED), left_out
    if left_out:
        print("systems left out (the reference did not converge them in 100 steps):", left_out)
    np.savez_compressed(os.path.join(mg.GOLD, "ccsd_systems.npz"), **{f"{t}__{k}": v for t, d in out.items() for k, v in d.items()})


if __name__ == "__main__":
    main()
