#!/usr/bin/env python3
"""Generate tests/golden/ccd_systems.npz: restricted LCCD and CCD of the REAL reference (needs oracle/_ref, `bash oracle/build_ref.sh`).

Per system of tests/golden/mp3_systems.npz (its C, eps and n_occ: the reference's own RHF orbitals at EXTREME convergence): the AO
integrals, the reference's AO->MO transformation (tuna_ci.py), then the reference's calculate_coupled_cluster_energy (tuna_cc.py:2950-3175)
with the functions it calls -- the LCCD and CCD amplitude updates, the energy expression, the convergence test, DIIS and damping --
executed from the source text, never copied.  Settings: energy convergence 1e-11, amplitude convergence 1e-10, DIIS with 6 vectors,
no damping, at most 100 steps.  Stored per system and method, all-electron (fc0) and with one frozen orbital (fc1): E_corr, n_iter, the
energy of every step (energies), ||t - t_old||_2 of every step (dt_norms) and the guess energy E_MP2.  n2_ccpvdz also has a NODIIS run
(nodiis_*) and a CORRDAMP 0.3 run (damp03_*), all-electron.  A system with a run the reference does not converge within 100 steps is
left out: of the six systems that is n2_sto3g, whose all-electron LCCD the reference gives up on after 100 steps (its CCD needs 77).
Only data is written.
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
from make_golden_mp3 import MP3_SYSTEMS  # noqa: E402

CC_FUNCTIONS = ("calculate_restricted_coupled_cluster_energy", "coupled_cluster_initial_print", "permute", "is_coupled_cluster_converged",
                "apply_damping", "update_DIIS", "apply_DIIS", "run_restricted_LCCD_iteration", "run_restricted_CCD_iteration",
                "calculate_coupled_cluster_energy")
REQUIRED = ("n2_ccpvdz", "n2_ccpvtz", "hf_ccpvdz", "ne_ccpvdz")


def _functions(path, names, ns):
    lines, _ = mg._parseable_lines(path)
    found = []
    for node in ast.parse("\n".join(lines)).body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module([node], []), os.path.basename(path), "exec"), ns)
            found.append(node.name)
    assert sorted(found) == sorted(names), (path, sorted(set(names) - set(found)))
    return ns


def load_reference_cc():
    """calculate_coupled_cluster_energy and what it calls from tuna_cc.py source text, with the tuna_mp / tuna_ci helpers they use.
    Returns (run, trace): trace["E"] and trace["dt"] collect the energy and ||t - t_old||_2 of every step of a run."""
    stubs = mg._stub_modules()["tuna_util"]
    base = {"np": np, "ndarray": np.ndarray, "Calculation": object, "Method": object, "Output": object, "Integrals": object, "Molecule": object,
            "log": stubs.log, "log_spacer": stubs.log_spacer, "timer": stubs.timer, "error": stubs.error}
    ci = types.SimpleNamespace(**{k: v for k, v in _functions(os.path.join(mg.REF, "TUNA", "tuna_ci.py"),
                                                              ("build_doubles_epsilons_tensor", "build_MP2_t_amplitudes"), dict(base)).items()
                                  if callable(v)})
    mp = types.SimpleNamespace(**{k: v for k, v in _functions(os.path.join(mg.REF, "TUNA", "tuna_mp.py"), ("calculate_restricted_MP2_energy",),
                                                              dict(base)).items() if callable(v)})
    ns = _functions(os.path.join(mg.REF, "TUNA", "tuna_cc.py"), CC_FUNCTIONS, dict(base, ci=ci, mp=mp))
    trace = {"E": [], "dt": []}
    energy, converged = ns["calculate_restricted_coupled_cluster_energy"], ns["is_coupled_cluster_converged"]

    def energy_traced(*a, **k):
        r = energy(*a, **k)
        trace["E"].append(float(r[0]))
        return r

    def converged_traced(delta_E, t, t_old, calculation):
        trace["dt"].append(float(np.linalg.norm(t[1] - t_old[1])))
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
            t_ijab = ci.build_MP2_t_amplitudes(g[o, o, v, v], e_ijab)          # tuna_cc.py:3268
            calc = types.SimpleNamespace(energy_convergence=1e-11, amp_conv=1e-10, correlated_max_iter=100, DIIS=diis, max_DIIS_matrices=6,
                                         correlated_damping_parameter=damping, reference="RHF")
            trace["E"].clear(); trace["dt"].clear()
            E_MP2 = float(mp.calculate_restricted_MP2_energy(t_ijab, g[o, o, v, v]))
            try:
                E_CC, _ = run_cc(g, o, v, (None, t_ijab, None, None), (None, e_ijab, None, None), np.diag(eps), types.SimpleNamespace(name=method),
                                 calc, True, None, None)
            except RuntimeError as e:                           # the reference's error(): not converged in 100 steps
                print("  left out:", tag, method, nf, diis, damping, e, flush=True)
                return None
            return dict(E_corr=float(E_CC), n_iter=len(trace["E"]), energies=np.array(trace["E"]), dt_norms=np.array(trace["dt"]), E_MP2=E_MP2)
        d, ok = {}, True
        for method in ("LCCD", "CCD"):
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
                print("CC", tag, pre, "E_corr", r["E_corr"], "steps", r["n_iter"], "last dE", r["energies"][-1] - r["energies"][-2], "last |dt|",
                      r["dt_norms"][-1], flush=True)
        if ok:
            out[tag] = d
        else:
            left_out.append(tag)
    assert all(t in out for t in REQUIRED), left_out
    if left_out:
        print("systems left out (the reference did not converge them in 100 steps):", left_out)
    np.savez_compressed(os.path.join(mg.GOLD, "ccd_systems.npz"), **{f"{t}__{k}": v for t, d in out.items() for k, v in d.items()})


if __name__ == "__main__":
    main()
