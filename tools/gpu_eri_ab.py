#!/usr/bin/env python3
"""GPU: A/B of the tensor build (tf_build_eri) between builds of the library, every call in a fresh child process that loads its library
through TUNAFOCK_LIB.

  [N | workload] name1 name2 ...   timing between library variants (tools/build_variant.sh; 'base' = tuna_amd/libtunafock.so, VAR=value[,..]
                       = the base library with that environment), alternating, twice: device time of the ERI kernels from the
                       library's own events (tf_eri_timings) and wall time of a warm rebuild, best of five builds.
  --time LIB_A LIB_B   the same child on synth-400, N2/cc-pVTZ and Ar2/cc-pVQZ in the order A, B, A', three times over.  Per row (ERI
                       kernels and wall time of each workload): the runs, the medians, the range of the six A / A' runs and whether
                       the B median lies within that range widened on each side by its own width.  One JSON line; exit status 1 if a
                       row is outside.
  --bits LIB_A LIB_B   the stored tensor byte for byte (SHA-256 of tf_copy_eri's output), tf_eri_build_stats and the counts of
                       tf_eri_timings for equality.  one_p, deep_p, high_l, n2_ccpvdz (tests/eri_shapes.py) and N2/cc-pVTZ on packed,
                       tiles and rows, spherical and Cartesian, TF_ERI_MODE=class and generic, each also with TF_SLAB_ROWS=1; then a
                       child each (packed) for TF_ERI_TEAMC=1, TF_ERI_TEAM=0, TF_ERI_GENERIC_OLD=1, TF_ERI_FAMILIES=1
                       TF_ERI_BRA_FAMILIES=1 and TF_ERI_NOFACT=1.  Per basis also tf_one_electron (S, T, V, D, Q), tf_cross_overlap and
                       tf_eri_element, hashed together.  LIB_A runs twice (A, A'): B must equal A wherever A equals A'.
Every child runs under its own time limit (--limit); the first child that fails or is killed ends the run, nothing is started after it.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
import bench
from tuna_amd.engine import Engine
atoms, shells, aos, nocc, desc = bench.build_workload(sys.argv[2])
with Engine(0) as eng:
    eng.set_basis(aos)
    best = None
    for rep in range(6):
        t0 = time.perf_counter(); eng.build_eri(True); wall = time.perf_counter() - t0
        t = eng.eri_timings()
        if rep and (best is None or t["cart_kernel_s"] < best["cart_kernel_s"]):
            best = dict(t, wall_s=wall)
    idx = np.random.default_rng(0).integers(0, eng.N, size=(2000, 4)).astype(np.int32)
    print(json.dumps({"eri_kernels_ms": 1e3 * best["cart_kernel_s"], "device_total_ms": 1e3 * best["total_s"], "wall_ms": 1e3 * best["wall_s"],
                      "checksum": float(np.abs(eng.sample_eri(idx)).sum())}))
"""
BITS_TAGS = ("one_p", "deep_p", "high_l", "n2_ccpvdz", "n2_ccpvtz")
BITS_VARIANTS = [("base", {}, ("packed", "tiles", "rows")), ("teamc", {"TF_ERI_TEAMC": "1"}, ("packed",)), ("team_off", {"TF_ERI_TEAM": "0"}, ("packed",)),
                 ("generic_old", {"TF_ERI_GENERIC_OLD": "1"}, ("packed",)),
                 ("families", {"TF_ERI_FAMILIES": "1", "TF_ERI_BRA_FAMILIES": "1"}, ("packed",)), ("nofact", {"TF_ERI_NOFACT": "1"}, ("packed",))]
COUNTS = ("shell_quartets", "primitive_shell_quartets", "component_quartets", "nominal_flops")


def child_bits(path, layouts):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import eri_shapes as es
    from tuna_amd import molecule as mol
    from tuna_amd.engine import Engine
    out = {}
    with Engine(0) as eng:
        for tag in BITS_TAGS:
            if tag == "n2_ccpvtz":
                aos = mol.expand_cartesian_aos(mol.build_shells(mol.make_atoms(["N", "N"], mol.angstrom_to_bohr(1.0977)), "cc-pVTZ"))
            else:
                aos = es.system(tag)[2]
            eng.set_basis(aos)
            # the entry points that need a basis and no tensor: tf_one_electron, tf_cross_overlap, tf_eri_element
            z = sorted({float(o[2]) for o in aos.origin})
            one = eng.one_electron([[0.0, 0.0, v] for v in z], [7.0] * len(z), [0.0, 0.0, 0.5 * z[-1]], spherical=False)
            n0 = int(aos.prim_off[1])                                         # (the first AO four times over)
            first4 = mol.AOList(aos.origin[:1].repeat(4, 0), aos.lmn[:1].repeat(4, 0), aos.nprim[:1].repeat(4), (n0 * np.arange(5)).astype(np.int32),
                                np.tile(aos.exps[:n0], 4), np.tile(aos.coefs[:n0], 4))
            h = hashlib.sha256(b"".join(m.tobytes() for m in one) + eng.cross_overlap(aos).tobytes() + np.float64(eng.eri_element(first4)).tobytes())
            out[f"{tag}.basis_entry_points"] = {"sha256": h.hexdigest(), "bytes": 0, "stats": {}, "counts": {}}
            for layout in layouts:
                for spherical in (True, False):
                    for mode in ("class", "generic"):
                        for rows in (None, "1"):
                            os.environ["TF_ERI_MODE"] = mode                   # (per-build knobs: read at every build)
                            os.environ.pop("TF_SLAB_ROWS", None)
                            if rows:
                                os.environ["TF_SLAB_ROWS"] = rows
                            eng.build_eri(spherical, layout=layout)
                            t = eng.eri_timings()
                            key = f"{tag}.{layout}.{'sph' if spherical else 'cart'}.{mode}.{'rows1' if rows else 'slab'}"
                            out[key] = {"sha256": hashlib.sha256(eng.copy_eri().tobytes()).hexdigest(), "bytes": 8 * eng.N ** 4,
                                        "stats": eng.eri_build_stats(), "counts": {k: t[k] for k in COUNTS}}
        eng._check(eng._L.tf_set_eri_layout(eng._ctx, -1))
    with open(path, "w") as f:
        json.dump(out, f)
    print(json.dumps({"builds": len(out)}))


def run_child(lib, args, limit, env=None):
    """one fresh process on one library, under its own time limit; None: it failed, and nothing more is to be started"""
    env = dict(os.environ, TUNAFOCK_LIB=os.path.abspath(lib), **(env or {}))
    try:
        p = subprocess.run([sys.executable] + args, env=env, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        print(f"STOP: the child on {lib} ran into its time limit of {limit} s; nothing more is started", flush=True)
        return None
    if p.returncode != 0 or not p.stdout.strip():
        print(f"STOP: the child on {lib} exited with {p.returncode}; nothing more is started\n{p.stderr[-2000:]}", flush=True)
        return None
    return json.loads(p.stdout.strip().splitlines()[-1])


def main_bits(a):
    report, bad = {}, False
    for name, env, layouts in BITS_VARIANTS:
        res = {}
        for run, lib in (("a", a.bits[0]), ("b", a.bits[1]), ("a2", a.bits[0])):
            path = os.path.join(a.out, f"eri_bits_{name}_{run}.json")
            if run_child(lib, [os.path.abspath(__file__), "--child", path, ",".join(layouts)], a.limit or 300, env) is None:
                return 1
            with open(path) as f:
                res[run] = json.load(f)
        assert sorted(res["a"]) == sorted(res["b"]) == sorted(res["a2"]), "the libraries made different sets of builds"
        unstable = [k for k in res["a"] if res["a"][k] != res["a2"][k]]
        differ = [k for k in res["a"] if k not in unstable and res["a"][k] != res["b"][k]]
        launches = {}
        for k, v in res["a"].items():
            for fam, n in v["stats"].items():
                launches[fam] = launches.get(fam, 0) + n
        report[name] = {"builds": len(res["a"]), "tensor_bytes": sum(v["bytes"] for v in res["a"].values()), "A_differs_from_A2": unstable,
                        "B_differs_from_A": differ, "launches_by_family": launches}
        bad = bad or bool(unstable or differ)
        print(name, json.dumps(report[name]), flush=True)
    print(json.dumps({"mode": "bits", "result": "DIFFERENT" if bad else "all equal", "children": report}))
    return 1 if bad else 0


def main_time(a):
    import numpy as np
    series = {"A": [], "B": [], "A'": []}
    for rep in range(3):
        for name, lib in (("A", a.time[0]), ("B", a.time[1]), ("A'", a.time[0])):
            row = {}
            for wl in ("synth-400", "n2-cc-pvtz", "ar2-cc-pvqz"):
                r = run_child(lib, ["-c", CHILD, ROOT, wl], a.limit or 300)
                if r is None:
                    return 1
                row[wl + " ERI kernels, ms"], row[wl + " warm rebuild wall, ms"], row[wl + " checksum"] = r["eri_kernels_ms"], r["wall_ms"], r["checksum"]
            series[name].append(row)
            print(name, rep, json.dumps(row), flush=True)
    out, ok = {"mode": "time", "what": "best of five warm rebuilds per process; medians of three processes"}, True
    for row in series["A"][0]:
        ref = [r[row] for r in series["A"] + series["A'"]]
        lo, hi = min(ref), max(ref)
        med = {name: float(np.median([r[row] for r in runs])) for name, runs in series.items()}
        inside = lo - (hi - lo) <= med["B"] <= hi + (hi - lo)
        out[row] = {"runs": {name: [r[row] for r in runs] for name, runs in series.items()}, "median": med, "range_A_A'": [lo, hi],
                    "within_widened_range": bool(inside)}
        ok = ok and inside
    print(json.dumps(out))
    return 0 if ok else 1


def main_variants(args):
    wl = args.pop(0) if args and (args[0].isdigit() or "-" in args[0]) else "400"
    if wl.isdigit():
        wl = "synth-" + wl
    names = args or ["base"]
    for rep in range(2):
        for name in names:
            # name = library variant, or VAR=value to run the base library with that environment variable (e.g. TF_ERI_FACT_THREADS=256)
            env = dict(os.environ)
            if "=" in name:
                for kv in name.split(","):                                  # VAR=value[,VAR2=value2...]
                    k, v = kv.split("=", 1)
                    env[k] = v
                lib = os.path.join(ROOT, "tuna_amd", "libtunafock.so")
            else:
                lib = os.path.join(ROOT, "tuna_amd", "libtunafock.so" if name == "base" else f"libtunafock_{name}.so")
            env["TUNAFOCK_LIB"] = lib
            out = subprocess.run([sys.executable, "-c", CHILD, ROOT, wl], env=env, capture_output=True, text=True)
            line = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else out.stderr[-600:]
            print(name, rep, line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", nargs=2, metavar="LIB")
    ap.add_argument("--time", nargs=2, metavar="LIB")
    ap.add_argument("--out", default=".")
    ap.add_argument("--limit", type=float, default=None, help="time limit of one child in seconds (default 300)")
    ap.add_argument("--child", nargs=2)
    ap.add_argument("names", nargs="*")
    a = ap.parse_args()
    if a.child:
        return child_bits(a.child[0], a.child[1].split(","))
    if a.bits or a.time:
        os.makedirs(a.out, exist_ok=True)
        return main_bits(a) if a.bits else main_time(a)
    return main_variants(a.names)


if __name__ == "__main__":
    sys.exit(main() or 0)
