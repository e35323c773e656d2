"""Records tests/golden/shard_plans.json: the owners that the library's tf_shard_plan_pairs / tf_shard_plan hand out for the cases of
tests/test_ctx_plan.py.  Run it against the library whose plans are to be pinned (TUNAFOCK_LIB names another build); no GPU is needed.
An owner array is stored run-length encoded, "rank x count" in order ("1x10 0x68"); where the free plan equals a forced one, its name
stands for it."""
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WORLDS = (1, 2, 3, 4, 8)
FORCED = ("", "segments", "shells")


def cases():
    from conftest import make_system
    from tuna_amd import molecule as mol
    out = {}
    for tag in ("n2_ccpvdz", "c3_ar2_ccpvqz"):
        out[tag] = [int(s.n_sph) for s in make_system(tag)[1]]
    atoms = mol.make_atoms(["AR", "AR"], 7.1)
    out["synthetic_400"] = [int(s.n_sph) for s in mol.build_shells(atoms, {18: mol.even_tempered_basis(*mol.synthetic_counts(400))})]
    out["one_shell"] = [5]
    out["all_equal"] = [3] * 7
    out["one_heavy"] = [1, 1, 3, 1, 1, 15, 1]
    return out


def rle(owner):
    return " ".join(f"{k}x{len(list(g))}" for k, g in itertools.groupby(owner.tolist()))


def main():
    from tuna_amd import _lib
    L = _lib.lib()
    doc = {"worlds": list(WORLDS), "forced": list(FORCED), "cases": {}}
    for name, dims in cases().items():
        dim = np.asarray(dims, dtype=np.int32)
        rec = {"dim": dims, "pairs": {}, "lpt": {}}
        for forced in FORCED:
            if forced:
                os.environ["TF_SHARD_PLAN"] = forced
            else:
                os.environ.pop("TF_SHARD_PLAN", None)
            for layout in (0, 1):
                for world in WORLDS:
                    owner = np.zeros(len(dim) * (len(dim) + 1) // 2, dtype=np.int32)
                    assert L.tf_shard_plan_pairs(len(dim), _lib.ptr(dim), layout, world, _lib.ptr(owner)) == 0
                    rec["pairs"][f"{forced or 'auto'}/{layout}/{world}"] = rle(owner)
        os.environ.pop("TF_SHARD_PLAN", None)
        for key in [k for k in rec["pairs"] if k.startswith("auto/")]:      # the free plan is one of the two
            same = [f for f in FORCED[1:] if rec["pairs"][f + key[4:]] == rec["pairs"][key]]
            assert same, key
            rec["pairs"][key] = same[0]
        w = dim.astype(np.int64) ** 2                      # the generic plan: any weights do
        for world in WORLDS:
            owner = np.zeros(len(w), dtype=np.int32)
            assert L.tf_shard_plan(len(w), _lib.ptr(w), world, _lib.ptr(owner)) == 0
            rec["lpt"][str(world)] = rle(owner)
        doc["cases"][name] = rec
    path = os.path.join(ROOT, "tests", "golden", "shard_plans.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
