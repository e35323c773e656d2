#!/usr/bin/env python3
"""Generate tests/golden/triples_systems.npz: the perturbative triples of the REAL reference (needs oracle/_ref, `bash oracle/build_ref.sh`).

Per system of tests/golden/mp3_systems.npz that tests/golden/ccsd_systems.npz holds (its C, eps and n_occ), all-electron (fc0) and with one
frozen orbital (fc1): the AO integrals and the reference's AO->MO transformation as in make_golden_ccsd.py / make_golden_mp4.py, then,
executed from the source text and never copied,
  MP4_fc{0,1}_E_T:            the third "ijab,ijab->" contraction of run_restricted_MP4 (tuna_mp.py:1552-1685) with the method name MP4,
                              i.e. with calculate_restricted_second_order_triples_amplitudes (tuna_mp.py:403-428);
  {CCSD,QCISD}_fc{0,1}_E_T:   calculate_restricted_CCSD_T_energy (tuna_cc.py:2688-2758) on the reference's own converged amplitudes of
                              calculate_coupled_cluster_energy with the thresholds of the CCSD goldens (1e-11, 1e-10, DIIS 6, no damping).
For co_631g and ne_ccpvdz also those converged amplitudes, {CCSD,QCISD}_fc{0,1}_t1 and _t2 (the other systems' would make the file large).
Host memory: the reference holds a handful of dense o^3 v^3 arrays, 0.4 GB each at N2/cc-pVTZ (o = 7, v = 53): 3-4 GB in all.  Only data
is written.
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
from make_golden_ccsd import load_reference_cc  # noqa: E402
from make_golden_mp3 import MP3_SYSTEMS  # noqa: E402

WITH_AMPLITUDES = ("co_631g", "ne_ccpvdz")


def load_reference_triples():
    """(run_restricted_MP3, run_restricted_MP4, components, calculate_restricted_CCSD_T_energy, build_triples_epsilons_tensor) from source
    text; components collects the scalars of run_restricted_MP4's final contractions of a call."""
    stubs = mg._stub_modules()["tuna_util"]
    base = {"np": np, "ndarray": np.ndarray, "Calculation": object, "Method": object, "log": stubs.log, "log_spacer": stubs.log_spacer,
            "timer": stubs.timer, "error": stubs.error}
    ci = types.SimpleNamespace(**{k: v for k, v in _functions(os.path.join(mg.REF, "TUNA", "tuna_ci.py"),
                                                              ("build_doubles_epsilons_tensor", "build_singles_epsilons_tensor",
                                                               "build_triples_epsilons_tensor"), dict(base)).items() if callable(v)})
    components = []

    class TracedNumpy:
        """numpy, with the full contractions "ijab,ijab->" recorded"""
        def __getattr__(self, name):
            return getattr(np, name)

        @staticmethod
        def einsum(spec, *a, **k):
            r = np.einsum(spec, *a, **k)
            if spec == "ijab,ijab->":
                components.append(float(r))
            return r
    mp_path = os.path.join(mg.REF, "TUNA", "tuna_mp.py")
    ns3 = _functions(mp_path, ("run_restricted_MP3",), dict(base, ci=ci))
    ns4 = _functions(mp_path, ("run_restricted_MP4", "permute_symmetric", "calculate_restricted_second_order_triples_amplitudes",
                               "permute_three_column_indices"), dict(base, ci=ci, np=TracedNumpy()))
    nst = _functions(os.path.join(mg.REF, "TUNA", "tuna_cc.py"), ("calculate_restricted_CCSD_T_energy",), dict(base, ci=ci))
    return ns3["run_restricted_MP3"], ns4["run_restricted_MP4"], components, nst["calculate_restricted_CCSD_T_energy"], ci.build_triples_epsilons_tensor


def main():
    assert mg.orc.ref_engine() is not None, "run oracle/build_ref.sh first"
    blocks, _ = mg.load_reference_kernel_bits()
    ao_to_mo, _ = mg.load_reference_ao_to_mo()
    run_mp3, run_mp4, components, ccsd_t, triples_eps = load_reference_triples()
    run_cc, _, ci, _ = load_reference_cc()
    z = np.load(os.path.join(mg.GOLD, "mp3_systems.npz"))
    held = {k.split("__", 1)[0] for k in np.load(os.path.join(mg.GOLD, "ccsd_systems.npz")).files}
    out = {}
    for tag, (sym, R, basis, nocc, _) in MP3_SYSTEMS.items():
        if tag not in held:
            continue
        C, eps = z[f"{tag}__C"], z[f"{tag}__eps"]
        assert int(z[f"{tag}__n_occ"]) == nocc
        atoms, shells, aos = mg.system(sym, R, basis)
        E = mg.one_e_and_eri(atoms, aos)[5]
        Es = mg.eri_to_spherical(mg.reference_U(shells, blocks), E)
        N = len(eps)
        g = ao_to_mo(Es, C, None, True)                              # chemists' (pq|rs)
        gp = g.swapaxes(1, 2)                                        # tuna_cc.py:3229: <pq|rs> = (pr|qs)
        d = {}
        for nf in (0, 1):
            o, v = slice(nf, nocc), slice(nocc, N)
            calc3 = types.SimpleNamespace(method=types.SimpleNamespace(name="MP3"), MP3_scaling=1 / 4)
            _, e_ijab, t_ijab, t_tilde_ijab, L = run_mp3(calc3, g, eps, 0.0, o, v, True)
            components.clear()
            run_mp4(e_ijab, t_ijab, t_tilde_ijab, L, g, eps, o, v, types.SimpleNamespace(method=types.SimpleNamespace(name="MP4")), True)
            assert len(components) == 4, components
            d[f"MP4_fc{nf}_E_T"] = components[2]
            print("T", tag, f"MP4 fc{nf}", components[2], flush=True)
            e_ijkabc = triples_eps(eps, o, v)
            for method in ("CCSD", "QCISD"):
                e2 = ci.build_doubles_epsilons_tensor(eps, eps, o, o, v, v)
                e1 = ci.build_singles_epsilons_tensor(eps, o, v)
                t2 = ci.build_MP2_t_amplitudes(gp[o, o, v, v], e2)
                calc = types.SimpleNamespace(energy_convergence=1e-11, amp_conv=1e-10, correlated_max_iter=100, DIIS=True, max_DIIS_matrices=6,
                                             correlated_damping_parameter=0.0, reference="RHF")
                E_CC, t = run_cc(gp, o, v, (np.zeros_like(e1), t2, None, None), (e1, e2, None, None), np.diag(eps), types.SimpleNamespace(name=method),
                                 calc, True, None, None)
                E_T = float(ccsd_t(gp, e_ijkabc, t[0], t[1], o, v, types.SimpleNamespace(name=f"{method}(T)"), calc, True))
                pre = f"{method}_fc{nf}_"
                d[pre + "E_T"], d[pre + "E_corr"] = E_T, float(E_CC)
                if tag in WITH_AMPLITUDES:
                    d[pre + "t1"], d[pre + "t2"] = np.array(t[0], dtype=float), np.array(t[1], dtype=float)
                print("T", tag, pre, "E_corr", float(E_CC), "E_T", E_T, flush=True)
        out[tag] = d
    np.savez_compressed(os.path.join(mg.GOLD, "triples_systems.npz"), **{f"{t}__{k}": v for t, d in out.items() for k, v in d.items()})


if __name__ == "__main__":
    main()
