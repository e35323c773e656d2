#!/usr/bin/env python3
"""Generate tests/golden/mp2_density_systems.npz: the MP2 one-particle densities of the REAL reference (needs oracle/_ref,
`bash oracle/build_ref.sh`).

Per system -- H2/STO-3G (o = v = 1), CO/STO-3G (v < o; N2/STO-3G, whose stored RHF solution has a singular A + B -- cond 3e16 -- fails
the conditioning check below and is not used), CO/6-31G, N2/cc-pVDZ, N2/cc-pVTZ (N = 60, all four parity classes) and F2/6-31G
(o = 9: o^2 = 81 pairs, one full batch of the ladder and a ragged one) -- the reference's own RHF orbitals at EXTREME convergence (those
of tests/golden/mp3_systems.npz where it has the system), then the reference's run_restricted_MP2 (tuna_mp.py:834-976) with everything
it calls -- calculate_restricted_relaxed_MP2_density_matrix, calculate_A_matrix / calculate_B_matrix, calculate_natural_orbitals,
spin_component_scale_MP2_energy -- and calculate_analytical_dipole_moment (tuna_props.py:96-121), executed from the source text, never
copied.  Stored per system: C, eps, n_occ, X, S, dipz (the z dipole matrix about the centre of mass), E_SCF, and per method (mp2;
scs = SCS-MP2 with the default scalings) E_OS, E_SS (unscaled), c_os, c_ss, the unrelaxed and relaxed P in the MO and AO bases
(<m>_P_mo_unrelaxed, ..._P_ao_relaxed), and for the relaxed case z, cond (of A + B), occ (natural occupations) and dipole (total,
nuclear, electronic); for the unrelaxed case occ_unrelaxed and dipole_unrelaxed.  text_<m>_<kind> holds what the reference prints
from "Constructing MP2 ..." to the end of the natural-occupation block for CO/6-31G.  Only data is written.
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
from tuna_amd import guess as guess_mod  # noqa: E402
from tuna_amd import molecule as mol  # noqa: E402

SYSTEMS = {"h2_sto3g": (["H", "H"], mol.angstrom_to_bohr(0.74), "STO-3G", 1, False),
           "co_sto3g": (["C", "O"], mol.angstrom_to_bohr(1.128), "STO-3G", 7, True),
           **{k: MP3_SYSTEMS[k] for k in ("co_631g", "n2_ccpvdz", "n2_ccpvtz")},
           "f2_631g": (["F", "F"], mol.angstrom_to_bohr(1.412), "6-31G", 9, True)}
METHODS = {"mp2": ("MP2", 1.0, 1.0), "scs": ("SCS-MP2", 6 / 5, 1 / 3)}        # name, c_os, c_ss (the reference's default OSS, SSS)
MP_FUNCTIONS = ("calculate_restricted_relaxed_MP2_density_matrix", "spin_component_scale_MP2_energy", "calculate_natural_orbitals",
                "run_restricted_MP2")


def load_reference_mp2_density():
    """run_restricted_MP2 and what it calls, from source text.  Returns (namespace, dipole function, stream, seen)."""
    stream, seen = [], {}

    def log(message, calculation=None, priority=1, silent=False, end="\n", colour=None):
        if not silent and priority <= 2:
            stream.append(message + end)
    stubs = mg._stub_modules()["tuna_util"]
    base = {"np": np, "ndarray": np.ndarray, "Calculation": object, "Molecule": object, "log": log, "log_spacer": lambda *a, **k: None,
            "timer": stubs.timer, "error": stubs.error, "symmetrise": stubs.symmetrise}
    ci_ns = _functions(os.path.join(mg.REF, "TUNA", "tuna_ci.py"), ("build_doubles_epsilons_tensor", "calculate_A_matrix", "calculate_B_matrix"), dict(base))
    A_ref, B_ref = ci_ns["calculate_A_matrix"], ci_ns["calculate_B_matrix"]

    def A_seen(*a, **k):
        seen["A"] = A_ref(*a, **k)
        return seen["A"]

    def B_seen(*a, **k):
        seen["B"] = B_ref(*a, **k)
        seen.setdefault("cond", []).append(float(np.linalg.cond(seen["A"] + seen["B"])))
        return seen["B"]
    ci = types.SimpleNamespace(build_doubles_epsilons_tensor=ci_ns["build_doubles_epsilons_tensor"], calculate_A_matrix=A_seen, calculate_B_matrix=B_seen)
    ns = _functions(os.path.join(mg.REF, "TUNA", "tuna_mp.py"), MP_FUNCTIONS, dict(base, ci=ci))
    relaxed_ref = ns["calculate_restricted_relaxed_MP2_density_matrix"]

    def relaxed_seen(P_unrelaxed, *a, **k):
        seen.setdefault("P_unrelaxed", []).append(P_unrelaxed.copy())
        P = relaxed_ref(P_unrelaxed, *a, **k)
        seen.setdefault("P_relaxed", []).append(P.copy())
        return P
    ns["calculate_restricted_relaxed_MP2_density_matrix"] = relaxed_seen
    props = _functions(os.path.join(mg.REF, "TUNA", "tuna_props.py"), ("calculate_nuclear_dipole_moment", "calculate_analytical_dipole_moment"), dict(base))
    return ns, props["calculate_analytical_dipole_moment"], stream, seen


def main():
    assert mg.orc.ref_engine() is not None, "run oracle/build_ref.sh first"
    blocks, ortho = mg.load_reference_kernel_bits()
    scf = mg.load_reference_scf()
    ao_to_mo, _ = mg.load_reference_ao_to_mo()
    ns, dipole_moment, stream, seen = load_reference_mp2_density()
    z3 = np.load(os.path.join(mg.GOLD, "mp3_systems.npz"))
    out = {}
    for tag, (sym, R, basis, nocc, damp) in SYSTEMS.items():
        atoms, shells, aos = mg.system(sym, R, basis)
        S, T, V, D, Q, E = mg.one_e_and_eri(atoms, aos)
        U = mg.reference_U(shells, blocks)
        Ss, Es = mg.to_spherical(U, S), mg.eri_to_spherical(U, E)
        com = guess_mod.centre_of_mass(atoms)
        xyz, chg = [a.origin for a in atoms], [float(a.charge) for a in atoms]
        Dcom = mg.orc.ref_one_electron(aos, xyz, chg, [0.0, 0.0, com])[3]
        dip = np.array([mg.to_spherical(U, d) for d in Dcom])
        X = ortho(Ss, None, True)[0]
        if f"{tag}__C" in z3.files:
            C, eps, E_SCF = z3[f"{tag}__C"], z3[f"{tag}__eps"], float(z3[f"{tag}__E_SCF"])
            assert int(z3[f"{tag}__n_occ"]) == nocc
        else:
            r = mg.run_reference_scf(scf, ortho, atoms, shells, Ss, mg.to_spherical(U, T), mg.to_spherical(U, V), Es, nocc, "extreme", damp)
            C, eps, E_SCF = r["C"], r["epsilons"], float(r["energy"])
        N = len(eps)
        g = ao_to_mo(Es, C, None, True)
        d = dict(C=C, eps=eps, n_occ=nocc, E_SCF=E_SCF, X=X, S=Ss, dipz=dip[2])
        molecule = types.SimpleNamespace(n_basis=N, n_doubly_occ=nocc)
        o, v = slice(0, nocc), slice(nocc, N)
        Cinv = C.T @ Ss                                          # C^-1 of S-orthonormal orbitals

        def run(name, c_os, c_ss, relaxed):
            calc = types.SimpleNamespace(method=types.SimpleNamespace(name=name), DFT_calculation=False, relaxed_density=relaxed, natural_orbitals=True,
                                         same_spin_scaling=c_ss, opposite_spin_scaling=c_os, HFX_prop=1.0, reference="RHF", MPC_requested=False, MPC_prop=1.0)
            stream.clear(); seen.clear()
            E_MP2, P, _, _, occ, _ = ns["run_restricted_MP2"](g, eps, C, o, v, X, calc, molecule, False, None, None)
            start = max(k for k, s in enumerate(stream) if "Constructing MP2" in s)
            text = "".join(stream[start:])
            mu = dipole_moment(com, np.array(chg), np.array(xyz), P, dip)
            return E_MP2, P, occ, np.array(mu, dtype=float), text
        gp = g.transpose(0, 2, 1, 3)[o, o, v, v]
        Dm = eps[o][:, None, None, None] + eps[o][None, :, None, None] - eps[v][None, None, :, None] - eps[v][None, None, None, :]
        d["E_OS"] = float(np.einsum("ijab,ijab->", gp, gp / Dm))
        d["E_SS"] = float(np.einsum("ijab,ijab->", gp, (gp - gp.swapaxes(2, 3)) / Dm))
        for m, (name, c_os, c_ss) in METHODS.items():
            E_u, P_u, occ_u, mu_u, text_u = run(name, c_os, c_ss, False)
            E_r, P_r, occ_r, mu_r, text_r = run(name, c_os, c_ss, True)
            assert abs(E_u - (c_os * d["E_OS"] + c_ss * d["E_SS"])) < 1e-12 and E_u == E_r
            ref2 = np.zeros((N, N)); ref2[o, o] = 2 * np.eye(nocc)
            Pmo_u = ref2 + c_os * seen["P_unrelaxed"][0] + c_ss * seen["P_unrelaxed"][1]
            Pmo_r = ref2 + c_os * seen["P_relaxed"][0] + c_ss * seen["P_relaxed"][1]
            assert np.abs(Cinv @ P_u @ Cinv.T - Pmo_u).max() < 1e-11 and np.abs(Cinv @ P_r @ Cinv.T - Pmo_r).max() < 1e-11
            zv = 2.0 * Pmo_r[o, v]
            cond = max(seen["cond"])
            # the room the 1e-10 tolerance of the GPU comparison has: an A + B this well conditioned loses nothing that matters in the solve
            assert cond * 1e-15 * np.abs(zv).max() < 1e-11, (tag, m, cond, np.abs(zv).max())
            d.update({f"{m}_c_os": c_os, f"{m}_c_ss": c_ss, f"{m}_P_mo_unrelaxed": Pmo_u, f"{m}_P_ao_unrelaxed": P_u, f"{m}_P_mo_relaxed": Pmo_r,
                      f"{m}_P_ao_relaxed": P_r, f"{m}_z": zv, f"{m}_cond": cond, f"{m}_occ": occ_r, f"{m}_dipole": mu_r, f"{m}_occ_unrelaxed": occ_u,
                      f"{m}_dipole_unrelaxed": mu_u})
            if tag == "co_631g":
                d[f"text_{m}_relaxed"], d[f"text_{m}_unrelaxed"] = np.array(text_r), np.array(text_u)
            print("MP2 density", tag, m, "N", N, "E", E_u, "cond(A+B)", cond, "max|z|", np.abs(zv).max(), "dipole", mu_r, "tr P", np.trace(Pmo_r), flush=True)
        out[tag] = d
    np.savez_compressed(os.path.join(mg.GOLD, "mp2_density_systems.npz"), **{f"{t}__{k}": val for t, d in out.items() for k, val in d.items()})


if __name__ == "__main__":
    main()
