#!/usr/bin/env python3
"""Generate tests/golden/mp4_systems.npz: restricted MP4(SDQ) and MP4(DQ) of the REAL reference (needs oracle/_ref, `bash oracle/build_ref.sh`).

Per system of tests/golden/mp3_systems.npz (its C, eps and n_occ: the reference's own RHF orbitals at EXTREME convergence): the AO
integrals, the reference's AO->MO transformation (tuna_ci.py), then the reference's run_restricted_MP3 and run_restricted_MP4
(tuna_mp.py:1418-1493, :1552-1685) executed from the source text, never copied.  run_restricted_MP4 returns the sum only and prints its
components to ten digits; the components stored here are the values of its own four final contractions
np.einsum("ijab,ijab->", t_tilde_ijab, X) (singles, doubles, triples, quadruples, in that order), read off the numpy namespace the
function runs in.  Stored per system, all-electron (fc0) and with one frozen orbital (fc1), for the levels SDQ and DQ:
{SDQ,DQ}_fc{0,1}_E_S, _E_D, _E_Q, _E_MP4 (the reference's own sum) and fc{0,1}_E_MP3.  Only data is written.
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


def load_reference_mp4():
    """(run_restricted_MP3, run_restricted_MP4, components) from tuna_mp.py source text with the tuna_ci helpers they call;
    components collects the scalars of run_restricted_MP4's final contractions of a call."""
    stubs = mg._stub_modules()["tuna_util"]
    base = {"np": np, "ndarray": np.ndarray, "Calculation": object, "log": stubs.log, "log_spacer": stubs.log_spacer, "timer": stubs.timer,
            "error": stubs.error}
    ci = types.SimpleNamespace(**{k: v for k, v in _functions(os.path.join(mg.REF, "TUNA", "tuna_ci.py"),
                                                              ("build_doubles_epsilons_tensor", "build_singles_epsilons_tensor"), dict(base)).items()
                                  if callable(v)})
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
    ns3 = _functions(os.path.join(mg.REF, "TUNA", "tuna_mp.py"), ("run_restricted_MP3",), dict(base, ci=ci))
    ns4 = _functions(os.path.join(mg.REF, "TUNA", "tuna_mp.py"), ("run_restricted_MP4", "permute_symmetric"), dict(base, ci=ci, np=TracedNumpy()))
    return ns3["run_restricted_MP3"], ns4["run_restricted_MP4"], components


def main():
    assert mg.orc.ref_engine() is not None, "run oracle/build_ref.sh first"
    blocks, _ = mg.load_reference_kernel_bits()
    ao_to_mo, _ = mg.load_reference_ao_to_mo()
    run_mp3, run_mp4, components = load_reference_mp4()
    z = np.load(os.path.join(mg.GOLD, "mp3_systems.npz"))
    out = {}
    for tag, (sym, R, basis, nocc, _) in MP3_SYSTEMS.items():
        C, eps = z[f"{tag}__C"], z[f"{tag}__eps"]
        assert int(z[f"{tag}__n_occ"]) == nocc
        atoms, shells, aos = mg.system(sym, R, basis)
        E = mg.one_e_and_eri(atoms, aos)[5]
        Es = mg.eri_to_spherical(mg.reference_U(shells, blocks), E)
        N = len(eps)
        g = ao_to_mo(Es, C, None, True)                              # chemists' (pq|rs), as run_restricted_MP3 takes it
        d = {}
        for nf in (0, 1):
            o, v = slice(nf, nocc), slice(nocc, N)
            calc3 = types.SimpleNamespace(method=types.SimpleNamespace(name="MP3"), MP3_scaling=1 / 4)
            E_MP3, e_ijab, t_ijab, t_tilde_ijab, L = run_mp3(calc3, g, eps, 0.0, o, v, True)
            d[f"fc{nf}_E_MP3"] = float(E_MP3)
            if nf == 0:
                assert abs(E_MP3 - float(z[f"{tag}__E_MP3"])) < 1e-12, (tag, E_MP3)
            for level in ("SDQ", "DQ"):
                calc4 = types.SimpleNamespace(method=types.SimpleNamespace(name=f"MP4({level})"))
                components.clear()
                E_MP4 = float(run_mp4(e_ijab, t_ijab, t_tilde_ijab, L, g, eps, o, v, calc4, True))
                assert len(components) == 4 and components[2] == 0.0, components
                E_S, E_D, _, E_Q = components
                assert E_MP4 == E_S + E_D + 0.0 + E_Q
                assert level == "SDQ" or E_S == 0.0
                pre = f"{level}_fc{nf}_"
                d.update({pre + "E_S": E_S, pre + "E_D": E_D, pre + "E_Q": E_Q, pre + "E_MP4": E_MP4})
                print("MP4", tag, pre, "E_S", E_S, "E_D", E_D, "E_Q", E_Q, "E_MP4", E_MP4, flush=True)
        out[tag] = d
    np.savez_compressed(os.path.join(mg.GOLD, "mp4_systems.npz"), **{f"{t}__{k}": v for t, d in out.items() for k, v in d.items()})


if __name__ == "__main__":
    main()
