#!/usr/bin/env python3
"""GPU timing of unrestricted Kohn-Sham: one tf_dft_vxc_unrestricted call against one tf_dft_vxc call on the same grid and the same
(total) density -- O2 / def2-TZVP, B3LYP, default ("medium") grid -- and the wall time of `SPE : O O 1.2075 : B3LYP DEF2-TZVP : ML 3`.
For the kernel list run it once more, on its own, under `rocprofv3 --kernel-trace --stats -- python tools/gpu_uks_timing.py --reps 3`."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tuna_amd import dft, molecule as mol  # noqa: E402
from tuna_amd.energy import run  # noqa: E402
from tuna_amd.engine import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    atoms = mol.make_atoms(["O", "O"], mol.angstrom_to_bohr(1.2075))
    shells = mol.build_shells(atoms, "def2-TZVP")
    with Engine(0) as eng:
        eng.set_basis(mol.expand_cartesian_aos(shells)).build_eri(True)
        pts, wts, info = dft.integration_grid(atoms, "medium")
        eng.dft_setup(pts, wts, "B3LYP")
        N = eng.N
        rng = np.random.default_rng(1)
        C = rng.standard_normal((N, 9)) * 0.3
        Pa = C @ C.T
        Pb = C[:, :7] @ C[:, :7].T
        for _ in range(3):                                           # warm-up (and the first-use allocation of the spin buffers)
            eng.dft_vxc(Pa + Pb)
            eng.dft_vxc_unrestricted(Pa, Pb)
        t = {}
        for name, fn in (("restricted", lambda: eng.dft_vxc(Pa + Pb)), ("unrestricted", lambda: eng.dft_vxc_unrestricted(Pa, Pb))):
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
            t[name] = float(np.median(ts))
        print(f"O2 / def2-TZVP B3LYP: N = {N}, G = {info['n_points']}")
        print(f"tf_dft_vxc              {t['restricted'] * 1e3:8.3f} ms per call (median of {a.reps}, host copies included)")
        print(f"tf_dft_vxc_unrestricted {t['unrestricted'] * 1e3:8.3f} ms per call  ratio {t['unrestricted'] / t['restricted']:.2f}")
    t0 = time.perf_counter()
    out = run("SPE : O O 1.2075 : B3LYP DEF2-TZVP : ML 3")
    wall = time.perf_counter() - t0
    print(f"SPE : O O 1.2075 : B3LYP DEF2-TZVP : ML 3  E = {out.energy:.10f}  iterations {out.n_iterations}  wall {wall:.2f} s")
    print("timings", {k: round(v, 4) for k, v in out.timings.items()})


if __name__ == "__main__":
    main()
