#!/usr/bin/env python3
"""Generate tests/golden/mp3_systems.npz: restricted MP3 of the REAL reference (needs oracle/_ref, `bash oracle/build_ref.sh`).

Per system: the reference's own RHF cycle from a core guess at EXTREME convergence (tools/make_golden.py run_reference_scf), its
AO->MO transformation (tuna_ci.py, as make_golden.make_mp2_golden), the MP2 spin components with the einsums of run_restricted_MP2
(tuna_mp.py:882-890), then the reference's run_restricted_MP3 (tuna_mp.py:1418-1493) executed from the source text.  Stored: C, eps,
n_occ, E_SCF, E_OS, E_SS, E_MP3; frozen-core variants with 1 and 2 frozen orbitals (fc1_*, fc2_*); the SCS-MP3 correlation energy at
the default scalings (scs_E_corr: SSS 1/3, OSS 6/5 on MP2, MP3S 1/4 on MP3, from the reference's SCS-MP3 run).  Only data is written.
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
# tag -> (symbols, R in bohr or None, basis, n_occ, damping)
MP3_SYSTEMS = {
    "n2_sto3g": (["N", "N"], A(1.0977), "STO-3G", 7, False),
    "n2_ccpvdz": (["N", "N"], A(1.0977), "cc-pVDZ", 7, False),
    "n2_ccpvtz": (["N", "N"], A(1.0977), "cc-pVTZ", 7, False),
    "co_631g": (["C", "O"], A(1.128), "6-31G", 7, True),
    "hf_ccpvdz": (["F", "H"], A(0.917), "cc-pVDZ", 5, False),
    "ne_ccpvdz": (["NE"], None, "cc-pVDZ", 5, False),
}


def load_reference_mp3():
    """run_restricted_MP3 from tuna_mp.py source text, with the tuna_ci helper it calls."""
    stubs = mg._stub_modules()["tuna_util"]
    ci = types.SimpleNamespace()
    ns_ci = {"np": np, "ndarray": np.ndarray, "Calculation": object, "log": stubs.log, "timer": stubs.timer, "error": stubs.error}
    for node in ast.parse(open(os.path.join(mg.REF, "TUNA", "tuna_ci.py")).read()).body:
        if isinstance(node, ast.FunctionDef) and node.name == "build_doubles_epsilons_tensor":
            exec(compile(ast.Module([node], []), "tuna_ci.py", "exec"), ns_ci)
            ci.build_doubles_epsilons_tensor = ns_ci[node.name]
    ns = {"np": np, "ndarray": np.ndarray, "Calculation": object, "ci": ci, "log": stubs.log, "log_spacer": stubs.log_spacer,
          "timer": stubs.timer, "error": stubs.error}
    lines, _ = mg._parseable_lines(os.path.join(mg.REF, "TUNA", "tuna_mp.py"))
    for node in ast.parse("\n".join(lines)).body:
        if isinstance(node, ast.FunctionDef) and node.name == "run_restricted_MP3":
            exec(compile(ast.Module([node], []), "tuna_mp.py", "exec"), ns)
    return ns["run_restricted_MP3"], ci.build_doubles_epsilons_tensor


def main():
    assert mg.orc.ref_engine() is not None, "run oracle/build_ref.sh first"
    scf = mg.load_reference_scf()
    blocks, ortho = mg.load_reference_kernel_bits()
    ao_to_mo, _ = mg.load_reference_ao_to_mo()
    run_mp3, doubles_eps = load_reference_mp3()
    out = {}
    for tag, (sym, R, basis, nocc, damp) in MP3_SYSTEMS.items():
        atoms, shells, aos = mg.system(sym, R, basis)
        S, T, V, D, Q, E = mg.one_e_and_eri(atoms, aos)
        U = mg.reference_U(shells, blocks)
        Ss, Ts_, Vs, Es = mg.to_spherical(U, S), mg.to_spherical(U, T), mg.to_spherical(U, V), mg.eri_to_spherical(U, E)
        r = mg.run_reference_scf(scf, ortho, atoms, shells, Ss, Ts_, Vs, Es, nocc, "extreme", damp)
        C, eps = r["C"], r["epsilons"]
        N = len(eps)
        g = ao_to_mo(Es, C, None, True)

        def energies(nf, method="MP3"):
            o, v = slice(nf, nocc), slice(nocc, N)
            e_ijab = doubles_eps(eps, eps, o, o, v, v)
            gp = g.transpose(0, 2, 1, 3)[o, o, v, v]                            # tuna_mp.py:882-890
            E_OS = float(np.einsum("ijab,ijab,ijab->", gp, gp, e_ijab, optimize=True))
            E_SS = float(np.einsum("ijab,ijab,ijab->", gp, gp - gp.swapaxes(2, 3), e_ijab, optimize=True))
            calc = types.SimpleNamespace(method=types.SimpleNamespace(name=method), MP3_scaling=1 / 4)
            E_MP2 = E_SS / 3 + 1.2 * E_OS if method == "SCS-MP3" else E_OS + E_SS
            E_MP3 = float(run_mp3(calc, g, eps, E_MP2, o, v, True)[0])
            return E_OS, E_SS, E_MP3, E_MP2 + E_MP3
        d = dict(C=C, eps=eps, n_occ=nocc, E_SCF=r["energy"])
        d["E_OS"], d["E_SS"], d["E_MP3"], _ = energies(0)
        for nf in (1, 2):
            d[f"fc{nf}_E_OS"], d[f"fc{nf}_E_SS"], d[f"fc{nf}_E_MP3"], _ = energies(nf)
        d["scs_E_corr"] = energies(0, "SCS-MP3")[3]
        out[tag] = d
        print("MP3", tag, N, "E_SCF", r["energy"], "E_MP2", d["E_OS"] + d["E_SS"], "E_MP3", d["E_MP3"], "SCS", d["scs_E_corr"], flush=True)
    np.savez_compressed(os.path.join(mg.GOLD, "mp3_systems.npz"), **{f"{t}__{k}": v for t, d in out.items() for k, v in d.items()})


if __name__ == "__main__":
    main()
