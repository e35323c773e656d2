#!/usr/bin/env python3
"""GPU: A/B of the correlated-method drivers (tf_ao_to_mo, tf_mp2_rhf ... tf_cis_rhf, tf_mp3_ladder_probe) between two builds of the
library, each call in a fresh child process that loads its library through TUNAFOCK_LIB, the processes alternating.  Like
gpu_jk_ab.py it stops at the first child that exits non-zero or is killed by its time limit and starts nothing after it.

  --bits LIB_A LIB_B   N2/cc-pVTZ (N = 60) with the golden orbitals of tests/golden/mp3_systems.npz on the packed, rows and tiles layouts:
                       every moved entry point once ((ov|ov) through tf_ao_to_mo; MP2; UMP2 on the same orbitals; MP3; MP4(DQ) and
                       MP4(SDQ); LCCD, CCD, LCCSD, QCISD, CCSD with 6 fixed steps, DIIS and damping 0.2; the three kinds of triples with
                       TF_TRIPLES_SLAB=3; CIS and TDHF, both multiplicities, with moments; the ladder probe on the packed layout).  Every
                       returned number and array except the seconds goes into one .npz per library; the two files are compared array by
                       array, byte for byte, and a difference is reported in units in the last place.
  --time LIB_A LIB_B   synth-400 (the bench workload) with its converged RHF orbitals, warm: MP3, MP4(SDQ), CCD and CCSD with 4 fixed steps
                       (as gpu_ccsd_timing.py runs them), then CIS and the MP4 triples at synth-200.  Order of the processes: A, B, A',
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


def converged_rhf(eng, atoms, shells, nocc):
    from tuna_amd import molecule as mol
    xyz, chg = [x.origin for x in atoms], [float(x.charge) for x in atoms]
    S, T, V, D, _ = eng.one_electron(xyz, chg, [0, 0, 0.5 * atoms[-1].origin[2]])
    X, _, _ = eng.orthogonaliser(S)
    _, C0 = eng.diagonalise(T + V, X)
    P0 = 2.0 * C0[:, :nocc] @ C0[:, :nocc].T
    nao = [sum(s.n_sph for s in shells if s.atom == k) for k in range(len(atoms))]
    r = eng.scf_rhf(S, T, V, 0.5 * (P0 + P0.T), float(np.sum(P0 * (T + V))), nocc, mol.nuclear_repulsion(atoms), X=X, conv="tight",
                    damping="dynamic", n_atom_ao=nao, max_iter=200)
    return r["C"], r["epsilons"], D


def flatten(prefix, r, out):
    for k, v in r.items():
        if k != "seconds" and v is not None:
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


def child_time():
    from tuna_amd import molecule as mol
    from tuna_amd.engine import Engine
    res = {}
    fixed = dict(max_iter=4, conv_delta_E=0.0, conv_amplitudes=0.0, allow_unconverged=True)
    with Engine(0) as eng:
        atoms, shells = synthetic(400)
        eng.set_basis(mol.expand_cartesian_aos(shells)).build_eri(True)
        C, eps, _ = converged_rhf(eng, atoms, shells, 18)
        calls = {"MP3": lambda: eng.mp3_rhf(C, eps, 18), "MP4(SDQ)": lambda: eng.mp4_rhf(C, eps, 18, level="SDQ"),
                 "CCD": lambda: eng.ccd_rhf(C, eps, 18, method="CCD", **fixed),
                 "CCSD": lambda: eng.ccsd_rhf(C, eps, 18, method="CCSD", return_t1=True, **fixed)}
        for name, call in calls.items():
            call()                                                # warm-up of this method's GEMM shapes
            res[name] = call()["seconds"][0]
        atoms, shells = synthetic(200)
        eng.set_basis(mol.expand_cartesian_aos(shells)).build_eri(True)
        C, eps, D = converged_rhf(eng, atoms, shells, 18)
        calls = {"CIS": lambda: eng.cis_rhf(C, eps, 18, method="CIS", n_keep=10, dip=D), "MP4 triples": lambda: eng.triples_rhf(C, eps, 18, kind="MP4")}
        for name, call in calls.items():
            call()
            res[name] = call()["seconds"][0]
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
    ap.add_argument("--child-time", action="store_true")
    a = ap.parse_args()
    if a.child_bits:
        return child_bits(a.child_bits)
    if a.child_time:
        return child_time()
    os.makedirs(a.out, exist_ok=True)
    if a.bits:
        files = [os.path.join(a.out, f"corr_bits_{name}.npz") for name in ("a", "b")]
        for lib, path in zip(a.bits, files):
            if run_child(lib, ["--child-bits", path], a.limit or 300) is None:
                return 1
        za, zb = np.load(files[0]), np.load(files[1])
        assert sorted(za.files) == sorted(zb.files), "the two libraries returned different sets of arrays"
        differ = {}
        for key in za.files:
            x, y = za[key], zb[key]
            if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
                differ[key] = ulps(x, y) if x.shape == y.shape and x.dtype == np.float64 else "shape or type"
        print(json.dumps({"mode": "bits", "arrays": len(za.files), "bytes": int(sum(za[k].nbytes for k in za.files)),
                          "result": "all equal" if not differ else "DIFFERENT", "max_ulps_of_the_arrays_that_differ": differ}))
        return 1 if differ else 0
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
