#!/usr/bin/env python3
"""GPU: A/B of the Fock build (tf_fock_jk, tf_fock_jk_device and the J/K hook of the native cycles) between two builds of the library,
each call in a fresh child process that loads its library through TUNAFOCK_LIB and runs under its own time limit.  Like
gpu_corr_ab.py it stops at the first child that exits non-zero or is killed by its time limit and starts nothing after it.

  --bits LIB_A LIB_B   J and K byte for byte.  Shapes two_s, one_p, c0_65, mid_17_9 (tests/fock_reference.py) and N2/cc-pVTZ on the
                       packed, tiles and rows layouts; calls of 1 and 2 symmetric densities, 1 non-symmetric and sym+nonsym+sym on every
                       layout, 4, 5, 8 and 9 symmetric on tiles.  The same in one child per variant, on the layout the variant acts on:
                       TF_JK_ONE_LAUNCH=0, TF_JK_ONE_LAUNCH=0 TF_JK_SERIAL=1, TF_JK_NOFUSE=1, TF_JK_PARTS=2 (packed), TF_TILE_PF=1 (tiles).
                       tf_fock_jk_device on a side stream (mid_17_9, packed and tiles, one and two densities).  One RHF and one UHF native
                       cycle on N2/cc-pVTZ with TF_JK_CD_NMIN=0, with their tf_jk_path_stats.  LIB_A runs twice (A, A'): B must equal A
                       wherever A equals A', and A must equal A' everywhere (nothing in these calls depends on timing).
  --time LIB_A LIB_B   seconds per Fock build through tf_fock_jk_device, warm, the device drained once after the last build.  synth-400:
                       packed with one density, two densities and one non-symmetric density; tiles with one and with eight densities
                       (mean of 20 builds).  N2/cc-pVTZ packed, one density: mean of 1000 back-to-back builds -- the launch-bound case,
                       where host overhead shows.  Processes in the order A, B, A', three times over.  Per row: the runs, the medians,
                       the range of the six A / A' runs, and whether the B median lies within that range widened on each side by its
                       own width.  Prints one JSON line; exit status 1 if a row is outside.

Usage: python tools/gpu_jk_ab.py (--bits | --time) LIB_A LIB_B [--out DIR] [--limit SECONDS]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

TAGS = ("two_s", "one_p", "c0_65", "mid_17_9", "n2_ccpvtz")
NONSYM = 9
CALLS = [("1 sym", [0]), ("2 sym", [0, 1]), ("1 nonsym", [NONSYM]), ("sym+nonsym+sym", [0, NONSYM, 1])]
CALLS_TILES = [("4 sym", [0, 1, 2, 3]), ("5 sym", [0, 1, 2, 3, 4]), ("8 sym", list(range(8))), ("9 sym", list(range(9)))]
VARIANTS = [("base", {}, ("packed", "tiles", "rows")), ("one_launch_0", {"TF_JK_ONE_LAUNCH": "0"}, ("packed",)),
            ("one_launch_0_serial", {"TF_JK_ONE_LAUNCH": "0", "TF_JK_SERIAL": "1"}, ("packed",)), ("nofuse", {"TF_JK_NOFUSE": "1"}, ("packed",)),
            ("parts_2", {"TF_JK_PARTS": "2"}, ("packed",)), ("tile_pf_1", {"TF_TILE_PF": "1"}, ("tiles",))]


def n2():
    from tuna_amd import molecule as mol
    atoms = mol.make_atoms(["N", "N"], mol.angstrom_to_bohr(1.0977))
    return atoms, mol.build_shells(atoms, "cc-pVTZ")


def aos_of(tag):
    import fock_reference as fr
    from tuna_amd import molecule as mol
    return mol.expand_cartesian_aos(n2()[1]) if tag == "n2_ccpvtz" else fr.system(tag)[2]


def pool(N):
    import fock_reference as fr
    S, G = fr.random_densities(N, NONSYM)
    return np.concatenate([S, G[None]])


def child_bits(path, layouts):
    from tuna_amd.engine import Engine
    out = {}
    with Engine(0) as eng:
        for tag in TAGS:
            for layout in layouts:
                eng.set_basis(aos_of(tag)).build_eri(True, layout=layout)
                assert eng.eri_storage()["layout"] == layout
                P = pool(eng.N)
                for name, idx in CALLS + (CALLS_TILES if layout == "tiles" else []):
                    J, K = eng.fock_jk(P[idx[0]] if len(idx) == 1 else P[idx])
                    out[f"{tag}.{layout}.{name}.J"], out[f"{tag}.{layout}.{name}.K"] = J, K
        eng._check(eng._L.tf_set_eri_layout(eng._ctx, -1))
    np.savez(path, **out)
    print(json.dumps({"arrays": len(out)}))


def child_device(path):
    import torch                                               # (torch initialises the device first: tests/test_gpu_fock_shapes.py)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    from tuna_amd.engine import Engine
    out = {}
    with Engine(0) as eng:
        for layout in ("packed", "tiles"):
            eng.set_basis(aos_of("mid_17_9")).build_eri(True, layout=layout)
            P = pool(eng.N)
            for nd in (1, 2):
                dP = torch.from_numpy(np.ascontiguousarray(P[:nd])).to("cuda:0")
                dJ, dK = torch.full_like(dP, float("nan")), torch.full_like(dP, float("nan"))
                torch.cuda.synchronize()
                eng.fock_jk_device(dP.data_ptr(), dJ.data_ptr(), dK.data_ptr(), nd, stream.cuda_stream)
                stream.synchronize()
                out[f"device.{layout}.{nd}.J"], out[f"device.{layout}.{nd}.K"] = dJ.cpu().numpy(), dK.cpu().numpy()
    np.savez(path, **out)
    print(json.dumps({"arrays": len(out)}))


def child_scf(path):
    from tuna_amd import molecule as mol
    from tuna_amd.engine import Engine
    atoms, shells = n2()
    out = {}
    with Engine(0) as eng:
        eng.set_basis(mol.expand_cartesian_aos(shells)).build_eri(True, layout="packed")
        xyz, chg = [x.origin for x in atoms], [float(x.charge) for x in atoms]
        S, T, V, _, _ = eng.one_electron(xyz, chg, [0, 0, 0.5 * atoms[-1].origin[2]])
        X, _, _ = eng.orthogonaliser(S)
        _, C0 = eng.diagonalise(T + V, X)
        Ph = C0[:, :7] @ C0[:, :7].T
        Ph = 0.5 * (Ph + Ph.T)
        E0, vnn = float(np.sum(2 * Ph * (T + V))), mol.nuclear_repulsion(atoms)
        nao = [sum(s.n_sph for s in shells if s.atom == k) for k in range(len(atoms))]
        kw = dict(X=X, conv="tight", damping="dynamic", n_atom_ao=nao)
        r = eng.scf_rhf(S, T, V, 2 * Ph, E0, 7, vnn, **kw)
        stats = eng.jk_path_stats()
        out.update({"rhf.energy": r["energy"], "rhf.n_iter": r["n_iter"], "rhf.P": r["P"], "rhf.F": r["F"], "rhf.table": np.asarray(r["table"])[:r["n_iter"]],
                    "rhf.path_stats": np.asarray(sorted(stats.items()), dtype=object).astype(str)})
        u = eng.scf_uhf(S, T, V, Ph, Ph, E0, 7, 7, vnn, **kw)
        stats = eng.jk_path_stats()
        out.update({"uhf.energy": u["energy"], "uhf.n_iter": u["n_iter"], "uhf.Pa": u["P_spin"][0], "uhf.Pb": u["P_spin"][1],
                    "uhf.table": np.asarray(u["table"])[:u["n_iter"]], "uhf.path_stats": np.asarray(sorted(stats.items()), dtype=object).astype(str)})
    np.savez(path, **{k: np.asarray(v) for k, v in out.items()})
    print(json.dumps({"arrays": len(out), "path_stats_after_uhf": stats}))


def child_time():
    import time
    import torch
    torch.cuda.set_device(0)
    from tuna_amd import molecule as mol
    from tuna_amd.engine import Engine
    res = {}

    def timed(eng, P, reps):
        nd = len(P)
        dP = torch.from_numpy(np.ascontiguousarray(P)).to("cuda:0")
        dJ, dK = torch.empty_like(dP), torch.empty_like(dP)
        for _ in range(max(3, reps // 10)):
            eng.fock_jk_device(dP.data_ptr(), dJ.data_ptr(), dK.data_ptr(), nd, 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            eng.fock_jk_device(dP.data_ptr(), dJ.data_ptr(), dK.data_ptr(), nd, 0)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps

    with Engine(0) as eng:
        atoms = mol.make_atoms(["AR", "AR"], 7.1)
        aos = mol.expand_cartesian_aos(mol.build_shells(atoms, {18: mol.even_tempered_basis(*mol.synthetic_counts(400))}))
        eng.set_basis(aos).build_eri(True, layout="packed")
        P = pool(eng.N)
        res["synth-400 packed 1"] = timed(eng, P[:1], 20)
        res["synth-400 packed 2"] = timed(eng, P[:2], 20)
        # (the device entry takes every density for symmetric; the host entry sends a non-symmetric one through two passes)
        t0 = time.perf_counter()
        for _ in range(20):
            eng.fock_jk(P[NONSYM])
        res["synth-400 packed 1 nonsym (host buffers)"] = (time.perf_counter() - t0) / 20
        eng.build_eri(True, layout="tiles")
        res["synth-400 tiles 1"] = timed(eng, P[:1], 20)
        res["synth-400 tiles 8"] = timed(eng, P[:8], 20)
        eng.set_basis(aos_of("n2_ccpvtz")).build_eri(True, layout="packed")
        res["n2_ccpvtz packed 1 (1000 builds)"] = timed(eng, pool(eng.N)[:1], 1000)
        eng._check(eng._L.tf_set_eri_layout(eng._ctx, -1))
    print(json.dumps(res))


def run_child(lib, args, limit, env=None):
    """one fresh process on one library, under its own time limit; None: it failed, and nothing more is to be started"""
    env = dict(os.environ, TUNAFOCK_LIB=os.path.abspath(lib), **(env or {}))
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        print(f"STOP: the child on {lib} ran into its time limit of {limit} s; nothing more is started", flush=True)
        return None
    if p.returncode != 0:
        print(f"STOP: the child on {lib} exited with {p.returncode}; nothing more is started\n{p.stderr[-2000:]}", flush=True)
        return None
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", nargs=2, metavar="LIB")
    ap.add_argument("--time", nargs=2, metavar="LIB")
    ap.add_argument("--out", default=".")
    ap.add_argument("--limit", type=float, default=None, help="time limit of one child in seconds (default 240 for --bits, 300 for --time)")
    ap.add_argument("--child", nargs="+")
    a = ap.parse_args()
    if a.child:
        kind, path = a.child[0], a.child[1] if len(a.child) > 1 else None
        return {"bits": lambda: child_bits(path, a.child[2].split(",")), "device": lambda: child_device(path), "scf": lambda: child_scf(path),
                "time": child_time}[kind]()
    os.makedirs(a.out, exist_ok=True)
    if a.bits:
        jobs = [(name, ["bits", None, ",".join(layouts)], env) for name, env, layouts in VARIANTS]
        jobs += [("device", ["device", None], {}), ("scf", ["scf", None], {"TF_JK_CD_NMIN": "0"})]
        report, bad = {}, False
        for name, args, env in jobs:
            files = {}
            for run, lib in (("a", a.bits[0]), ("b", a.bits[1]), ("a2", a.bits[0])):
                files[run] = os.path.join(a.out, f"jk_bits_{name}_{run}.npz")
                info = run_child(lib, ["--child", args[0], files[run]] + args[2:], a.limit or 240, env)
                if info is None:
                    return 1
            za, zb, za2 = (np.load(files[r]) for r in ("a", "b", "a2"))
            assert sorted(za.files) == sorted(zb.files) == sorted(za2.files), "the libraries returned different sets of arrays"
            same = lambda x, y: x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
            unstable = [k for k in za.files if not same(za[k], za2[k])]
            differ = [k for k in za.files if k not in unstable and not same(za[k], zb[k])]
            report[name] = {"arrays": len(za.files), "bytes": int(sum(za[k].nbytes for k in za.files)), "A_differs_from_A2": unstable, "B_differs_from_A": differ}
            if name == "scf":
                report[name]["path_stats"] = {k: za[k].tolist() for k in za.files if k.endswith("path_stats")}
            bad = bad or bool(unstable or differ)
            print(name, json.dumps(report[name]), flush=True)
        print(json.dumps({"mode": "bits", "result": "DIFFERENT" if bad else "all equal", "children": report}))
        return 1 if bad else 0
    if a.time:
        series = {"A": [], "B": [], "A'": []}
        for rep in range(3):
            for name, lib in (("A", a.time[0]), ("B", a.time[1]), ("A'", a.time[0])):
                r = run_child(lib, ["--child", "time"], a.limit or 300)
                if r is None:
                    return 1
                series[name].append(r)
                print(name, rep, json.dumps(r), flush=True)
        out, ok = {"mode": "time", "what": "seconds per Fock build; medians of three processes"}, True
        for row in series["A"][0]:
            ref = [r[row] for r in series["A"] + series["A'"]]
            lo, hi = min(ref), max(ref)
            med = {name: float(np.median([r[row] for r in runs])) for name, runs in series.items()}
            inside = lo - (hi - lo) <= med["B"] <= hi + (hi - lo)
            out[row] = {"runs": {name: [r[row] for r in runs] for name, runs in series.items()}, "median": med, "range_A_A'": [lo, hi],
                        "B_over_A": med["B"] / med["A"], "within_widened_range": bool(inside)}
            ok = ok and inside
        print(json.dumps(out))
        return 0 if ok else 1
    ap.error("one of --bits and --time")


if __name__ == "__main__":
    sys.exit(main() or 0)
