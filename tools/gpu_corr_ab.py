#!/usr/bin/env python3
"""GPU: A/B of the correlated-method and excited-state drivers (tf_ao_to_mo, tf_mp2_rhf ... tf_cis_rhf, tf_mp3_ladder_probe; tf_cis_uhf,
tf_tddft_rhf / _uhf, tf_xc_kernel_rhf / _uhf, tf_stability_*, tf_cis_d_rhf) between two builds of the library, each call in a fresh child
process that loads its library through TUNAFOCK_LIB, the processes alternating.  Like gpu_jk_ab.py it stops at the first child that
exits non-zero or is killed by its time limit and starts nothing after it.

  --bits LIB_A LIB_B   N2/cc-pVTZ (N = 60) with the golden orbitals of tests/golden/mp3_systems.npz on the packed, rows and tiles layouts:
                       every moved entry point once ((ov|ov) through tf_ao_to_mo; MP2; UMP2 on the same orbitals; MP3; MP4(DQ) and
                       MP4(SDQ); LCCD, CCD, LCCSD, QCISD, CCSD with 6 fixed steps, DIIS and damping 0.2; the three kinds of triples with
                       TF_TRIPLES_SLAB=3; CIS and TDHF, both multiplicities, with moments; the ladder probe on the packed layout).  A second
                       child, on stored systems of tests/golden (ucis_systems, tddft_systems, utddft_systems, cis_systems; open shells
                       with o_alpha != o_beta and with an empty beta block; the grids set up as tests/test_gpu_tddft.py does): cis_uhf CIS
                       and TDHF; tddft_rhf and tddft_uhf, TDA and full, with hfx = 0 and 0.2; xc_kernel_rhf / _uhf with their point
                       values; stability_rhf / _uhf / _rks / _uks with spectra and modes; cis_d_rhf.  A call the library refuses goes in
                       with its message.  Every returned number and array except the seconds goes into one .npz per process.  As in
                       gpu_jk_ab.py LIB_A runs twice (A, A'): an array on which A does not reproduce itself is listed by name and not
                       compared; every other one must be B's byte for byte, and a difference is reported in units in the last place.
  --time LIB_A LIB_B   synth-400 (the bench workload) with its converged RHF orbitals, warm: MP3, MP4(SDQ), CCD and CCSD with 4 fixed steps
                       (as gpu_ccsd_timing.py runs them), then at synth-200 CIS and the MP4 triples, cis_rhf TDHF, cis_uhf TDHF with
                       (o_alpha, o_beta) = (10, 8) (the shapes and the shift of gpu_ucis_timing.py) and, on the LDA Kohn-Sham orbitals
                       and the medium grid of gpu_utddft_timing.py, full-response tddft_rhf, tddft_uhf with 8 and 10 orbitals frozen,
                       and stability_rks (a call the library refuses is reported as refused).  Order of the processes: A, B, A',
                       three times over, A' being LIB_A again: per method the seconds[0] of each run, the medians of the three series and
                       the A-against-A' spread that B is to be read against.  Prints one JSON line.

Usage: python tools/gpu_corr_ab.py (--bits | --time) LIB_A LIB_B [--out DIR] [--limit SECONDS]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic(n):
    from tuna_amd import molecule as mol
    atoms = mol.make_atoms(["AR", "AR"], 7.1)
    return atoms, mol.build_shells(atoms, {18: mol.even_tempered_basis(*mol.synthetic_counts(n))})


def converged_rhf(eng, atoms, shells, nocc, **scf):
    from tuna_amd import molecule as mol
    xyz, chg = [x.origin for x in atoms], [float(x.charge) for x in atoms]
    S, T, V, D, _ = eng.one_electron(xyz, chg, [0, 0, 0.5 * atoms[-1].origin[2]])
    X, _, _ = eng.orthogonaliser(S)
    _, C0 = eng.diagonalise(T + V, X)
    P0 = 2.0 * C0[:, :nocc] @ C0[:, :nocc].T
    nao = [sum(s.n_sph for s in shells if s.atom == k) for k in range(len(atoms))]
    r = eng.scf_rhf(S, T, V, 0.5 * (P0 + P0.T), float(np.sum(P0 * (T + V))), nocc, mol.nuclear_repulsion(atoms), X=X, conv="tight",
                    damping="dynamic", n_atom_ao=nao, max_iter=200, **scf)
    return r["C"], r["epsilons"], D, r["P"]


def flatten(prefix, r, out):
    for k, v in r.items():
        if isinstance(v, dict):
            flatten(f"{prefix}.{k}", v, out)
        elif k != "seconds" and v is not None:
            out[f"{prefix}.{k}"] = np.asarray(v)


def child_bits(path):
    from tuna_amd import molecule as mol
    from tuna_amd.engine import Engine
    z = np.load(os.path.join(ROOT, "tests", "golden", "mp3_systems.npz"))
    C, eps, nocc = z["n2_ccpvtz__C"], z["n2_ccpvtz__eps"], 7
    atoms = mol.make_atoms(["N", "N"], mol.angstrom_to_bohr(1.0977))
    aos = mol.expand_cartesian_aos(mol.build_shells(atoms, "cc-pVTZ"))
    os.environ["TF_TRIPLES_SLAB"] = "3"
    fixed = dict(max_iter=6, conv_delta_E=0.0, conv_amplitudes=0.0, allow_unconverged=True, use_diis=True, damping=0.2, return_t2=True)
    out = {}
    with Engine(0) as eng:
        for layout in ("packed", "rows", "tiles"):
            eng.set_basis(aos).build_eri(True, layout=layout)
            assert eng.eri_storage()["layout"] == layout
            xyz, chg = [x.origin for x in atoms], [float(x.charge) for x in atoms]
            D = eng.one_electron(xyz, chg, [0, 0, 0.5 * atoms[-1].origin[2]])[3]
            Co, Cv = np.ascontiguousarray(C[:, :nocc]), np.ascontiguousarray(C[:, nocc:])
            out[f"{layout}.ao_to_mo.ovov"] = eng.ao_to_mo(Co, Cv, Co, Cv)
            flatten(f"{layout}.mp2", eng.mp2_rhf(C, eps, nocc), out)
            flatten(f"{layout}.ump2", eng.mp2_uhf(C, C, eps, eps, nocc, nocc), out)
            flatten(f"{layout}.mp3", eng.mp3_rhf(C, eps, nocc), out)
            for level in ("DQ", "SDQ"):
                flatten(f"{layout}.mp4_{level}", eng.mp4_rhf(C, eps, nocc, level=level), out)
            for method in ("LCCD", "CCD"):
                flatten(f"{layout}.{method}", eng.ccd_rhf(C, eps, nocc, method=method, **fixed), out)
            amps = {}
            for method in ("LCCSD", "QCISD", "CCSD"):
                amps[method] = eng.ccsd_rhf(C, eps, nocc, method=method, return_t1=True, **fixed)
                flatten(f"{layout}.{method}", amps[method], out)
            for kind, src in (("CCSD(T)", "CCSD"), ("QCISD(T)", "QCISD"), ("MP4", None)):
                kw = dict(t1=amps[src]["t1"], t2=amps[src]["t2"]) if src else {}
                flatten(f"{layout}.triples_{kind}", eng.triples_rhf(C, eps, nocc, kind=kind, return_e_ijk=True, **kw), out)
            for method in ("CIS", "TDHF"):
                flatten(f"{layout}.{method}", eng.cis_rhf(C, eps, nocc, method=method, n_keep=5, dip=D, return_matrices=True), out)
            if layout == "packed":
                T = np.random.default_rng(5).standard_normal((70, eng.N, eng.N))
                out["packed.ladder_probe"] = eng.mp3_ladder_probe(T)
        eng._check(eng._L.tf_set_eri_layout(eng._ctx, -1))
    np.savez(path, **out)
    print(json.dumps({"arrays": len(out)}))


def child_excited(path):
    """the excited-state and stability drivers on stored systems; a refusal of the library is a result (its code and message are kept)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_cis_reference as tc
    import test_ucis_reference as tu
    import xc_kernel_reference as xk
    import xc_kernel_spin_reference as xs
    from tuna_amd import dft
    from tuna_amd._lib import TunaError
    from tuna_amd.engine import Engine
    golden = lambda name: tc.split(np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")))
    out = {}

    def keep(prefix, call):
        try:
            r = call()
            flatten(prefix, r if isinstance(r, dict) else {str(k): v for k, v in enumerate(r)}, out)
        except TunaError as e:
            out[prefix + ".refused"] = np.asarray(f"{e.code}: {e}")

    def grid(eng, atoms, aos, level, functional):
        eng.set_basis(aos).build_eri(True)
        pts, wts, _ = dft.integration_grid(atoms, level)
        eng.dft_setup(np.asarray(pts, float).reshape(3, -1), np.asarray(wts, float).reshape(-1), functional)

    with Engine(0) as eng:
        # unrestricted Hartree-Fock: o_alpha != o_beta (9, 7), an unstable reference, an empty beta block
        g = golden("ucis_systems")
        for tag in ("o2_triplet_ccpvdz", "o2_triplet_sto3g", "li_doublet_631g", "h_ccpvdz"):
            eng.set_basis(tu.usystem(tag)[1]).build_eri(True)
            orb, win = tu.orbitals(g[tag]), tu.windows(g[tag])
            for method in ("CIS", "TDHF"):
                keep(f"{tag}.cis_uhf_{method}", lambda: eng.cis_uhf(*orb, *win, method=method, n_keep=4, dip=g[tag]["dip"], return_matrices=True))
            keep(f"{tag}.stability_uhf", lambda: eng.stability_uhf(*orb, *win, return_spectra=True, return_mode=True))
        # restricted Hartree-Fock: the stability analysis, and CIS(D) of the four lowest CIS states of either multiplicity
        g = golden("cis_systems")["n2_ccpvdz"]
        eng.set_basis(tc.system("n2_ccpvdz")[1]).build_eri(True)
        C, eps, nocc = g["C"], g["eps"], int(g["n_occ"])
        keep("n2_ccpvdz.stability_rhf", lambda: eng.stability_rhf(C, eps, nocc, return_spectra=True, return_mode=True))
        cis = eng.cis_rhf(C, eps, nocc, method="CIS", n_keep=4)
        for k, mult in enumerate(("singlet", "triplet")):
            keep(f"n2_ccpvdz.cis_d_{mult}", lambda: eng.cis_d_rhf(C, eps, nocc, b=cis["X_" + mult], omega=cis["E_" + mult][:4], triplet=[k] * 4))
        # restricted Kohn-Sham, local-density functionals
        g = golden("tddft_systems")
        for tag in ("lih_svwn3_sto3g", "hf_svwn_631g", "co_lda_631g"):
            atoms, _, aos = xk.system(tag)
            grid(eng, atoms, aos, xk.SYSTEMS[tag][5], xk.SYSTEMS[tag][4])
            C, eps, P, nocc = g[tag]["C"], g[tag]["eps"], g[tag]["P"], int(g[tag]["n_occ"])
            for method in ("TDA", "TDDFT"):
                for hfx in (0.0, 0.2):
                    keep(f"{tag}.tddft_rhf_{method}_hfx{hfx}", lambda: eng.tddft_rhf(C, eps, P, nocc, method=method, hfx=hfx, n_keep=4, dip=g[tag]["dip"],
                                                                                       return_matrices=True))
            keep(f"{tag}.xc_kernel_rhf", lambda: eng.xc_kernel_rhf(C, P, nocc, return_points=True))
            for hfx in (None, 0.0):
                keep(f"{tag}.stability_rks_hfx{hfx}", lambda: eng.stability_rks(C, eps, P, nocc, hfx=hfx, return_spectra=True, return_mode=True))
        # unrestricted Kohn-Sham: (5, 3), (2, 1), an empty beta block (1, 0), and a reference past its spin-symmetry breaking point
        g = golden("utddft_systems")
        for tag in ("nh_svwn3_sto3g", "li_svwn3_631g", "h_lda_631g", "lih_stretched_lda_sto3g"):
            atoms, _, aos = xs.system(tag)
            grid(eng, atoms, aos, xs.SYSTEMS[tag][6], xs.SYSTEMS[tag][5])
            orb, dens, win = tu.orbitals(g[tag]), (g[tag]["P_alpha"], g[tag]["P_beta"]), (int(g[tag]["n_alpha"]), int(g[tag]["n_beta"]))
            for method in ("TDA", "TDDFT"):
                for hfx in (0.0, 0.2):
                    keep(f"{tag}.tddft_uhf_{method}_hfx{hfx}", lambda: eng.tddft_uhf(*orb, *dens, *win, method=method, hfx=hfx, n_keep=4, dip=g[tag]["dip"],
                                                                                       return_matrices=True))
            keep(f"{tag}.xc_kernel_uhf", lambda: eng.xc_kernel_uhf(orb[0], orb[1], *dens, *win, return_points=True))
            for hfx in (None, 0.0):
                keep(f"{tag}.stability_uks_hfx{hfx}", lambda: eng.stability_uks(*orb, *dens, *win, hfx=hfx, return_spectra=True, return_mode=True))
        eng.dft_clear()
    np.savez(path, **out)
    print(json.dumps({"arrays": len(out), "refused": sorted(k for k in out if k.endswith(".refused"))}))


def child_time():
    from tuna_amd import dft, molecule as mol
    from tuna_amd._lib import TunaError
    from tuna_amd.engine import Engine
    res = {}
    fixed = dict(max_iter=4, conv_delta_E=0.0, conv_amplitudes=0.0, allow_unconverged=True)
    with Engine(0) as eng:
        atoms, shells = synthetic(400)
        eng.set_basis(mol.expand_cartesian_aos(shells)).build_eri(True)
        C, eps, _, _ = converged_rhf(eng, atoms, shells, 18)
        calls = {"MP3": lambda: eng.mp3_rhf(C, eps, 18), "MP4(SDQ)": lambda: eng.mp4_rhf(C, eps, 18, level="SDQ"),
                 "CCD": lambda: eng.ccd_rhf(C, eps, 18, method="CCD", **fixed),
                 "CCSD": lambda: eng.ccsd_rhf(C, eps, 18, method="CCSD", return_t1=True, **fixed)}
        for name, call in calls.items():
            call()                                                # warm-up of this method's GEMM shapes
            res[name] = call()["seconds"][0]
        atoms, shells = synthetic(200)
        eng.set_basis(mol.expand_cartesian_aos(shells)).build_eri(True)
        C, eps, D, _ = converged_rhf(eng, atoms, shells, 18)
        ea, eb = eps.copy(), eps.copy()                       # (o_alpha, o_beta) = (10, 8) on the closed-shell orbitals, the virtual energies of
        ea[10:] += 30.0                                       # either spin 30 Eh higher: gpu_ucis_timing.py
        eb[8:] += 30.0
        calls = {"CIS": lambda: eng.cis_rhf(C, eps, 18, method="CIS", n_keep=10, dip=D), "MP4 triples": lambda: eng.triples_rhf(C, eps, 18, kind="MP4"),
                 "cis_rhf TDHF": lambda: eng.cis_rhf(C, eps, 18, method="TDHF", n_keep=10, dip=D),
                 "cis_uhf TDHF": lambda: eng.cis_uhf(C, C, ea, eb, 10, 8, method="TDHF", n_keep=10, dip=D)}
        for name, call in calls.items():
            call()
            res[name] = call()["seconds"][0]
        pts, wts, _ = dft.integration_grid(atoms, "medium")   # LDA Kohn-Sham on the medium grid, 8 alpha and 10 beta orbitals frozen:
        hfx = eng.dft_setup(pts, wts, "LDA")["hfx"]           # gpu_utddft_timing.py
        C, eps, D, P = converged_rhf(eng, atoms, shells, 18, hfx=hfx)
        calls = {"tddft_rhf TDDFT": lambda: eng.tddft_rhf(C, eps, P, 18, method="TDDFT", n_keep=10, dip=D),
                 "tddft_uhf TDDFT": lambda: eng.tddft_uhf(C, C, eps, eps, P / 2, P / 2, 18, 18, 8, 10, method="TDDFT", n_keep=10, dip=D),
                 "stability_rks": lambda: eng.stability_rks(C, eps, P, 18, 0)}
        for name, call in calls.items():
            try:
                call()
                res[name] = call()["seconds"][0]
            except TunaError as e:                            # an unstable reference: reported, not timed
                res[name] = "refused: " + str(e)[:160]
        eng.dft_clear()
    print(json.dumps(res))


def run_child(lib, args, limit):
    """one fresh process on one library, under its own time limit; None: it failed, and nothing more is to be started"""
    env = dict(os.environ, TUNAFOCK_LIB=os.path.abspath(lib))
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        print(f"STOP: the child on {lib} ran into its time limit of {limit} s; nothing more is started", flush=True)
        return None
    if p.returncode != 0:
        print(f"STOP: the child on {lib} exited with {p.returncode}; nothing more is started\n{p.stderr[-2000:]}", flush=True)
        return None
    return json.loads(p.stdout.strip().splitlines()[-1])


def ulps(a, b):
    a, b = np.ascontiguousarray(a, float).ravel(), np.ascontiguousarray(b, float).ravel()
    ia, ib = a.view(np.int64).copy(), b.view(np.int64).copy()
    ia[ia < 0] = np.iinfo(np.int64).min - ia[ia < 0]          # the order of the reals on the integers
    ib[ib < 0] = np.iinfo(np.int64).min - ib[ib < 0]
    return int(np.abs(ia.astype(np.float64) - ib.astype(np.float64)).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", nargs=2, metavar="LIB")
    ap.add_argument("--time", nargs=2, metavar="LIB")
    ap.add_argument("--out", default=".")
    ap.add_argument("--limit", type=float, default=None, help="time limit of one child in seconds (default 300 for --bits, 420 for --time)")
    ap.add_argument("--child-bits")
    ap.add_argument("--child-excited")
    ap.add_argument("--child-time", action="store_true")
    a = ap.parse_args()
    if a.child_bits:
        return child_bits(a.child_bits)
    if a.child_excited:
        return child_excited(a.child_excited)
    if a.child_time:
        return child_time()
    os.makedirs(a.out, exist_ok=True)
    if a.bits:
        same = lambda x, y: x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        report, bad = {}, False
        for kind in ("bits", "excited"):                         # one fresh child per kind and library, in the order A, B, A'
            files = {}
            for run, lib in (("a", a.bits[0]), ("b", a.bits[1]), ("a2", a.bits[0])):
                files[run] = os.path.join(a.out, f"corr_{kind}_{run}.npz")
                if run_child(lib, [f"--child-{kind}", files[run]], a.limit or 300) is None:
                    return 1
            za, zb, za2 = (np.load(files[r]) for r in ("a", "b", "a2"))
            assert sorted(za.files) == sorted(zb.files) == sorted(za2.files), "the libraries returned different sets of arrays"
            unstable = sorted(k for k in za.files if not same(za[k], za2[k]))
            differ = {k: ulps(za[k], zb[k]) if za[k].shape == zb[k].shape and za[k].dtype == zb[k].dtype == np.float64 else "shape, type or text"
                      for k in za.files if k not in unstable and not same(za[k], zb[k])}
            report[kind] = {"arrays": len(za.files), "bytes": int(sum(za[k].nbytes for k in za.files)), "compared": len(za.files) - len(unstable),
                            "A_differs_from_A2_not_compared": unstable, "max_ulps_of_the_arrays_that_differ": differ,
                            "refused": sorted(k for k in za.files if k.endswith(".refused"))}
            bad = bad or bool(differ)
            print(kind, json.dumps(report[kind]), flush=True)
        print(json.dumps({"mode": "bits", "result": "DIFFERENT" if bad else "all equal", "children": report}))
        return 1 if bad else 0
    if a.time:
        series = {"A": [], "B": [], "A'": []}
        for rep in range(3):
            for name, lib in (("A", a.time[0]), ("B", a.time[1]), ("A'", a.time[0])):
                r = run_child(lib, ["--child-time"], a.limit or 420)
                if r is None:
                    return 1
                series[name].append(r)
                print(name, rep, json.dumps(r), flush=True)
        out = {"mode": "time", "what": "seconds[0] per method; medians of three processes"}
        for method in series["A"][0]:
            if any(not isinstance(r[method], float) for runs in series.values() for r in runs):       # refused somewhere: no statistics
                out[method] = {"runs": {name: [r[method] for r in runs] for name, runs in series.items()}}
                continue
            med = {name: float(np.median([r[method] for r in runs])) for name, runs in series.items()}
            out[method] = {"runs": {name: [r[method] for r in runs] for name, runs in series.items()}, "median": med,
                           "B_over_A": med["B"] / med["A"], "Aprime_over_A": med["A'"] / med["A"],
                           "within_spread": abs(med["B"] - med["A"]) <= max(abs(med["A'"] - med["A"]),
                                                                            max(r[method] for r in series["A"] + series["A'"]) -
                                                                            min(r[method] for r in series["A"] + series["A'"]))}
        print(json.dumps(out))
        return 0
    ap.error("one of --bits and --time")


if __name__ == "__main__":
    sys.exit(main() or 0)
