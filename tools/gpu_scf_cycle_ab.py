#!/usr/bin/env python3
"""GPU: A/B of the native SCF cycles (tf_scf_rhf, tf_scf_rhf_batch, tf_scf_uhf, tf_scf_uks) between two builds of the library, each
call in a fresh child process that loads its library through TUNAFOCK_LIB.  Like gpu_corr_ab.py it stops at the first child that exits
non-zero or is killed by its time limit and starts nothing after it.

  --bits LIB_A LIB_B   every number and array the cycles return except the seconds (energy, components, table, n_iter, converged, rc, P, F,
                       C, eps and their per-spin versions), one .npz per process.  Restricted, packed layout: N2/STO-3G (n = 10) and
                       N2/cc-pVDZ (28) (the fused n <= 64 paths), N2/cc-pVTZ (60), Ar2/cc-pVQZ (118, blocked refinement), synth-200
                       (refinement as the library chooses it; the report says which), each with damping none / dynamic / fixed 0.3,
                       max_diis 2 and 6, DIIS off, a field term and a run cut off at max_iter = 3; N2/cc-pVTZ once more on tiles; one RKS run
                       (N2/6-31G, BLYP) and, on the same tensor, tf_dft_vxc and tf_dft_vxc_unrestricted themselves (SVWN, BLYP, B3LYP; the loose
                       grid whole and cut to 127, 128, 129 and 12 801 points; each call twice and once after a fresh set-up); UHF on the O2 triplet (STO-3G, cc-pVDZ), the Li doublet, the H atom and the Li quartet (both n_beta = 0) in 6-31G and,
                       above n = 64, the NO doublet in cc-pVQZ with damping on and off and the Ar2+ doublet in cc-pVQZ (118; blocks <= 64: the
                       blocked refinement in both spin slots); tf_orthogonaliser and tf_diagonalise themselves on a context without a tensor
                       (n = 2, 33, 64, 65, 100) and on the n40_blocked, mmax64 and mmax65 tensors of tests/test_gpu_eigh.py with class-diagonal
                       random matrices of a fixed seed, each call twice; UKS on the golden O2 triplet B3LYP/STO-3G; a lockstep
                       batch of three field cycles.  Every run also records what tf_eigh_stats and tf_jk_path_stats counted during it.
                       LIB_A runs twice (A, A'): B is compared byte for byte with A on every array on which A and A' agree byte for
                       byte.  Only arrays of the lockstep batch may be left out that way; those are compared with the tolerance
                       tests/test_host_logic.py has for the batch (energies to 1e-10, equal iteration counts).
  --time LIB_A LIB_B   warm, in the process order A, B, A', three times over: the two SCF legs of bench.py (synth-400, TIGHT, DIIS 6 with the
                       bench's fall-back to dynamic damping; N2/cc-pVTZ, EXTREME, no damping), one UHF cycle (synth-200 triplet), one UKS
                       cycle (O2 triplet B3LYP/cc-pVDZ) and one RKS cycle (CO B3LYP/def2-TZVP, medium grid: BASELINE config 4): wall_seconds, fock_seconds and eig_seconds of each, the medians of the three series
                       and the A-against-A' spread B is to be read against.  Prints one JSON line.

Usage: python tools/gpu_scf_cycle_ab.py (--bits | --time) LIB_A LIB_B [--out DIR] [--limit SECONDS]
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
SECONDS = ("fock_seconds", "eig_seconds", "wall_seconds")


def system(symbols, R_angstrom, basis):
    from tuna_amd import molecule as mol
    atoms = mol.make_atoms(symbols, None if R_angstrom is None else mol.angstrom_to_bohr(R_angstrom))
    return atoms, mol.build_shells(atoms, basis)


def synthetic(n):
    from tuna_amd import molecule as mol
    atoms = mol.make_atoms(["AR", "AR"], 7.1)
    return atoms, mol.build_shells(atoms, {18: mol.even_tempered_basis(*mol.synthetic_counts(n))})


def prepare(eng, atoms, shells, layout=None):
    """tensor, integrals, X and the core orbitals, all from the device (as bench.py prepares its legs)"""
    from tuna_amd import molecule as mol
    eng.set_basis(mol.expand_cartesian_aos(shells)).build_eri(True, layout=layout)
    xyz, chg = [a.origin for a in atoms], [float(a.charge) for a in atoms]
    S, T, V, D, _ = eng.one_electron(xyz, chg, [0, 0, 0.5 * atoms[-1].origin[2] if len(atoms) == 2 else 0.0])
    X, _, _ = eng.orthogonaliser(S)
    _, C0 = eng.diagonalise(T + V, X)
    nao = [sum(s.n_sph for s in shells if s.atom == k) for k in range(len(atoms))]
    return S, T, V, D, X, C0, nao, mol.nuclear_repulsion(atoms)


def guess(C0, T, V, n, per_orbital):
    P = per_orbital * C0[:, :n] @ C0[:, :n].T
    return 0.5 * (P + P.T), float(np.sum(P * (T + V)))


class Recorder:
    """runs a cycle, keeps everything it returns but the seconds (also from a failed call: its partial result and code) and the paths it took"""

    def __init__(self, eng):
        self.eng, self.out, self.paths = eng, {}, {}

    def __call__(self, name, call):
        from tuna_amd._lib import TunaError
        e0, j0 = self.eng.eigh_stats(), self.eng.jk_path_stats()
        try:
            res, rc = call(), 0
        except TunaError as err:
            res, rc = err.partial, err.code
        for k, r in enumerate(res if isinstance(res, list) else [res]):
            prefix = f"{name}[{k}]" if isinstance(res, list) else name
            for key, v in r.items():
                if key not in SECONDS and v is not None:
                    self.out[f"{prefix}.{key}"] = np.asarray(v)
            self.out[f"{prefix}.return_code"] = np.asarray(rc)
        e1, j1 = self.eng.eigh_stats(), self.eng.jk_path_stats()
        self.paths[name] = {k: e1[k] - e0[k] for k in e0 if e1[k] != e0[k]} | {k: j1[k] - j0[k] for k in j0 if j1[k] != j0[k]}


def restricted_runs(rec, eng, tag, S, T, V, D, X, C0, nao, vnn, nocc, conv):
    P0, E0 = guess(C0, T, V, nocc, 2.0)
    kw = dict(X=X, conv=conv, n_atom_ao=nao)
    runs = {"nodamp": dict(damping="none"), "dynamic": dict(damping="dynamic"), "static0.3": dict(damping="static", damping_factor=0.3),
            "diis2": dict(damping="dynamic", max_diis=2), "nodiis": dict(damping="dynamic", diis=False, max_iter=40),
            "field": dict(damping="dynamic", Fext=0.002 * D[2]), "cut3": dict(damping="dynamic", max_iter=3)}
    for name, extra in runs.items():
        rec(f"{tag}.{name}", lambda: eng.scf_rhf(S, T, V, P0, E0, nocc, vnn, **{**kw, **extra}))
    return P0, E0, kw


def direct_vxc(out, eng, atoms):
    """tf_dft_vxc and tf_dft_vxc_unrestricted themselves on the tensor the engine holds (N2/6-31G): SVWN, BLYP and B3LYP on the loose grid
    whole and cut to 127, 128, 129 and 12 801 points in random order (the split-K edges of the V assembly), random PSD densities, every
    call twice, and once more after dft_clear + dft_setup; everything returned is kept"""
    from tuna_amd import dft
    pts, wts = dft.integration_grid(atoms, "loose")[:2]
    pts, wts = np.asarray(pts).reshape(3, -1), np.asarray(wts).reshape(-1)
    rng = np.random.default_rng(5)
    psd = [c @ c.T / c.shape[1] for c in (rng.standard_normal((eng.N, k)) for k in (7, 6, 4))]
    P, Pa, Pb = psd[0], 0.5 * psd[1], 0.3 * psd[2]

    def keep(name, res):
        for k, v in enumerate(res):
            out[f"{name}.{k}"] = np.asarray(v)

    for functional in ("SVWN", "BLYP", "B3LYP"):
        for G in (None, 127, 128, 129, 12801):
            idx = slice(None) if G is None else np.random.default_rng(G).permutation(wts.size)[:G]
            p, w = np.ascontiguousarray(pts[:, idx]), np.ascontiguousarray(wts[idx])
            assert G is None or w.size == G
            tag = f"vxc.{functional}.{'whole' if G is None else G}"
            eng.dft_setup(p, w, functional)
            for rep in ("first", "second"):
                keep(f"{tag}.restricted.{rep}", eng.dft_vxc(P))
                keep(f"{tag}.unrestricted.{rep}", eng.dft_vxc_unrestricted(Pa, Pb))
            eng.dft_clear()
            eng.dft_setup(p, w, functional)
            keep(f"{tag}.unrestricted.fresh", eng.dft_vxc_unrestricted(Pa, Pb))
            keep(f"{tag}.restricted.fresh", eng.dft_vxc(P))
            eng.dft_clear()


# the parity-block configurations of tests/test_gpu_eigh.py: (s, p, d, f) shells of an even-tempered basis on N and on O
EIGH_CONFIGS = {"n40_blocked": ((5, 3, 1, 0), (7, 3, 1, 0)), "mmax64": ((20, 12, 0, 0), (20, 12, 0, 0)), "mmax65": ((20, 12, 0, 0), (21, 12, 0, 0))}


def direct_eigh(rec, eng, tag, mats):
    """tf_orthogonaliser and tf_diagonalise themselves (X = 1: eps, C of the matrix; then X = S^-1/2 of a positive matrix), each call
    twice: a second solve on tables and blocks that the first one left"""
    for k, A in enumerate(mats):
        n = A.shape[0]
        S = A @ A.T / n + 1e-2 * np.eye(n)
        S = 0.5 * (S + S.T)
        for rep in ("first", "second"):
            rec(f"eigh.{tag}.{k}.diagonalise.{rep}", lambda: dict(zip(("eps", "C"), eng.diagonalise(A, np.eye(n)))))
            rec(f"eigh.{tag}.{k}.orthogonaliser.{rep}", lambda: dict(zip(("X", "smallest", "S_inv"), eng.orthogonaliser(S))))
        X = eng.orthogonaliser(S)[0]
        rec(f"eigh.{tag}.{k}.diagonalise.X", lambda: dict(zip(("eps", "C"), eng.diagonalise(A, X))))


def child_eigh(out, paths):
    from tuna_amd import molecule as mol
    from tuna_amd.engine import Engine
    rng = np.random.default_rng(4)
    with Engine(0) as eng:                                        # no tensor: no symmetry offered, the full-matrix paths
        rec = Recorder(eng)
        for n in (2, 33, 64, 65, 100):
            g = rng.standard_normal((n, n))
            direct_eigh(rec, eng, f"plain.n{n}", [0.5 * (g + g.T)])
        out.update(rec.out); paths.update(rec.paths)
    for name, (ca, cb) in EIGH_CONFIGS.items():                   # a tensor's parity classes: class-diagonal matrices go block by block
        atoms = mol.make_atoms(["N", "O"], 2.2)
        shells = mol.build_shells(atoms, {7: mol.even_tempered_basis(*ca), 8: mol.even_tempered_basis(*cb)})
        with Engine(0) as eng:
            rec = Recorder(eng)
            eng.set_basis(mol.expand_cartesian_aos(shells)).build_eri(True)
            U, lmn = eng.sph_matrix(), np.asarray(eng.aos.lmn)
            c_cart = (lmn[:, 0] & 1) | ((lmn[:, 1] & 1) << 1)
            cls = np.array([c_cart[np.flatnonzero(np.abs(U[i]) > 1e-12)[0]] for i in range(U.shape[0])])
            mats = []
            for _ in range(2):
                g = rng.standard_normal((eng.N, eng.N))
                mats.append(0.5 * (g + g.T) * (cls[:, None] == cls[None, :]))
            direct_eigh(rec, eng, name, mats)
            out.update(rec.out); paths.update(rec.paths)


def child_bits(path):
    from tuna_amd import dft
    from tuna_amd.engine import Engine
    eigh_out, eigh_paths = {}, {}
    child_eigh(eigh_out, eigh_paths)
    with Engine(0) as eng:
        rec = Recorder(eng)
        rec.out.update(eigh_out); rec.paths.update(eigh_paths)
        sizes = [("n2_sto3g", system(["N", "N"], 1.0977, "STO-3G"), 7, "extreme"), ("n2_ccpvdz", system(["N", "N"], 1.0977, "cc-pVDZ"), 7, "extreme"),
                 ("n2_ccpvtz", system(["N", "N"], 1.0977, "cc-pVTZ"), 7, "extreme"), ("ar2_ccpvqz", system(["AR", "AR"], 3.76, "cc-pVQZ"), 18, "tight"),
                 ("synth200", synthetic(200), 18, "tight")]
        for tag, (atoms, shells), nocc, conv in sizes:
            S, T, V, D, X, C0, nao, vnn = prepare(eng, atoms, shells, "packed")
            P0, E0, kw = restricted_runs(rec, eng, tag, S, T, V, D, X, C0, nao, vnn, nocc, conv)
            if tag == "n2_ccpvtz":
                fields = [None, 0.002 * D[2], -0.002 * D[2]]
                rec("batch.n2_ccpvtz", lambda: eng.scf_rhf_batch(S, T, V, [P0] * 3, [E0] * 3, nocc, vnn, Fexts=fields, damping="dynamic", **kw))
        atoms, shells = system(["N", "N"], 1.0977, "cc-pVTZ")
        S, T, V, D, X, C0, nao, vnn = prepare(eng, atoms, shells, "tiles")
        assert eng.eri_storage()["layout"] == "tiles"
        restricted_runs(rec, eng, "tiles.n2_ccpvtz", S, T, V, D, X, C0, nao, vnn, 7, "extreme")
        eng._check(eng._L.tf_set_eri_layout(eng._ctx, -1))

        atoms, shells = system(["N", "N"], 1.0977, "6-31G")                    # restricted Kohn-Sham
        S, T, V, D, X, C0, nao, vnn = prepare(eng, atoms, shells)
        f = eng.dft_setup(*dft.integration_grid(atoms, "loose")[:2], "BLYP")
        P0, E0 = guess(C0, T, V, 7, 2.0)
        rec("rks.n2_631g_blyp", lambda: eng.scf_rhf(S, T, V, P0, E0, 7, vnn, X=X, conv="extreme", hfx=f["hfx"], n_atom_ao=nao))
        eng.dft_clear()
        direct_vxc(rec.out, eng, atoms)

        uhf = [("o2_sto3g", (["O", "O"], 1.2075, "STO-3G"), 9, 7, ("dynamic", "none")), ("o2_ccpvdz", (["O", "O"], 1.2075, "cc-pVDZ"), 9, 7, ("dynamic",)),
               ("li_631g", (["LI"], None, "6-31G"), 2, 1, ("dynamic", "none")), ("h_631g", (["H"], None, "6-31G"), 1, 0, ("dynamic", "none")),
               ("li_quartet_631g", (["LI"], None, "6-31G"), 3, 0, ("dynamic",)),
               ("no_ccpvqz", (["N", "O"], 1.151, "cc-pVQZ"), 8, 7, ("dynamic", "none")),
               ("ar2plus_ccpvqz", (["AR", "AR"], 3.76, "cc-pVQZ"), 18, 17, ("dynamic",))]   # blocks <= 64: the blocked refinement in both spin slots
        for tag, spec, na, nb, dampings in uhf:
            atoms, shells = system(*spec)
            S, T, V, D, X, C0, nao, vnn = prepare(eng, atoms, shells)
            (Pa, Ea), (Pb, Eb) = guess(C0, T, V, na, 1.0), guess(C0, T, V, nb, 1.0)
            for damping in dampings:
                rec(f"uhf.{tag}.{damping}", lambda: eng.scf_uhf(S, T, V, Pa, Pb, Ea + Eb, na, nb, vnn, X=X, conv="tight" if eng.N > 64 else "extreme",
                                                                damping=damping, n_atom_ao=nao, max_iter=200))
            if tag == "li_631g":
                rec(f"uhf.{tag}.diis2", lambda: eng.scf_uhf(S, T, V, Pa, Pb, Ea + Eb, na, nb, vnn, X=X, conv="extreme", damping="none", max_diis=2, n_atom_ao=nao))

        g = np.load(os.path.join(ROOT, "tests", "golden", "uks_systems.npz"))    # unrestricted Kohn-Sham on a golden system
        tag = "o2_b3lyp_sto3g"
        from tuna_amd import molecule as mol
        atoms = mol.make_atoms([str(x) for x in g[tag + "__symbols"]], float(g[tag + "__R"]))
        shells = mol.build_shells(atoms, str(g[tag + "__basis"]))
        S, T, V, D, X, C0, nao, vnn = prepare(eng, atoms, shells)
        f = eng.dft_setup(*dft.integration_grid(atoms, str(g[tag + "__grid"]))[:2], str(g[tag + "__functional"]))
        na, nb = int(g[tag + "__n_alpha"]), int(g[tag + "__n_beta"])
        rec("uks." + tag, lambda: eng.scf_uks(S, T, V, g[tag + "__P0_alpha"], g[tag + "__P0_beta"], float(g[tag + "__E0"]), na, nb, vnn, X=X,
                                              conv="extreme", damping="dynamic", hfx=f["hfx"], n_atom_ao=nao, max_iter=int(g[tag + "__max_iter"])))
        eng.dft_clear()
    np.savez(path, **rec.out)
    print(json.dumps({"arrays": len(rec.out), "paths": rec.paths}))


def child_time():
    from tuna_amd import dft
    from tuna_amd._lib import TunaError
    from tuna_amd.engine import Engine
    res = {}

    def timed(name, call):
        call()                                                    # warm-up of this cycle's GEMM shapes and solvers
        r = call()
        res[name] = {k: r[k] for k in SECONDS} | {"n_iter": r["n_iter"]}

    with Engine(0) as eng:
        atoms, shells = synthetic(400)                            # bench.py: scf_on_workload
        S, T, V, D, X, C0, nao, vnn = prepare(eng, atoms, shells)
        P0, E0 = guess(C0, T, V, 18, 2.0)

        def leg400():
            try:
                return eng.scf_rhf(S, T, V, P0, E0, 18, vnn, X=X, conv="tight", damping="none", n_atom_ao=nao, max_iter=100)
            except TunaError:
                return eng.scf_rhf(S, T, V, P0, E0, 18, vnn, X=X, conv="tight", damping="dynamic", n_atom_ao=nao, max_iter=200)
        timed("rhf synth-400 tight", leg400)

        atoms, shells = system(["N", "N"], 1.0977, "cc-pVTZ")     # bench.py: scf_leg
        S1, T1, V1, D, X1, C1, nao1, vnn1 = prepare(eng, atoms, shells)
        P1, E1 = guess(C1, T1, V1, 7, 2.0)
        timed("rhf n2/cc-pvtz extreme", lambda: eng.scf_rhf(S1, T1, V1, P1, E1, 7, vnn1, X=X1, conv="extreme", damping="none", n_atom_ao=[30, 30]))

        atoms, shells = synthetic(200)
        S2, T2, V2, D, X2, C2, nao2, vnn2 = prepare(eng, atoms, shells)
        (Pa, Ea), (Pb, Eb) = guess(C2, T2, V2, 19, 1.0), guess(C2, T2, V2, 17, 1.0)
        timed("uhf synth-200 triplet", lambda: eng.scf_uhf(S2, T2, V2, Pa, Pb, Ea + Eb, 19, 17, vnn2, X=X2, conv="tight", damping="dynamic", n_atom_ao=nao2,
                                                           max_iter=200))

        atoms, shells = system(["O", "O"], 1.2075, "cc-pVDZ")
        S3, T3, V3, D, X3, C3, nao3, vnn3 = prepare(eng, atoms, shells)
        f = eng.dft_setup(*dft.integration_grid(atoms, "loose")[:2], "B3LYP")
        (Pa3, Ea3), (Pb3, Eb3) = guess(C3, T3, V3, 9, 1.0), guess(C3, T3, V3, 7, 1.0)
        timed("uks o2/cc-pvdz b3lyp", lambda: eng.scf_uks(S3, T3, V3, Pa3, Pb3, Ea3 + Eb3, 9, 7, vnn3, X=X3, conv="tight", damping="dynamic", hfx=f["hfx"],
                                                          n_atom_ao=nao3, max_iter=200))
        eng.dft_clear()

        atoms, shells = system(["C", "O"], 1.128, "def2-TZVP")     # BASELINE config 4
        S4, T4, V4, D, X4, C4, nao4, vnn4 = prepare(eng, atoms, shells)
        f = eng.dft_setup(*dft.integration_grid(atoms, "medium")[:2], "B3LYP")
        P4, E4 = guess(C4, T4, V4, 7, 2.0)
        timed("rks co/def2-tzvp b3lyp", lambda: eng.scf_rhf(S4, T4, V4, P4, E4, 7, vnn4, X=X4, conv="tight", damping="dynamic", hfx=f["hfx"],
                                                            n_atom_ao=nao4, max_iter=200))
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


def same(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


def ulps(a, b):
    a, b = np.ascontiguousarray(a, float).ravel(), np.ascontiguousarray(b, float).ravel()
    ia, ib = a.view(np.int64).copy(), b.view(np.int64).copy()
    ia[ia < 0] = np.iinfo(np.int64).min - ia[ia < 0]          # the order of the reals on the integers
    ib[ib < 0] = np.iinfo(np.int64).min - ib[ib < 0]
    return int(np.abs(ia.astype(np.float64) - ib.astype(np.float64)).max()) if a.size else 0


def compare_bits(files, infos):
    za, za2, zb = (np.load(f) for f in files)
    assert sorted(za.files) == sorted(za2.files) == sorted(zb.files), "the processes returned different sets of arrays"
    unstable = [k for k in za.files if not same(za[k], za2[k])]
    differ = {k: (ulps(za[k], zb[k]) if za[k].shape == zb[k].shape and za[k].dtype == np.float64 else "shape or type")
              for k in za.files if k not in unstable and not same(za[k], zb[k])}
    outside_batch = [k for k in unstable if not k.startswith("batch.")]
    loose = {}
    for k in unstable:                                         # the lockstep batch where A and A' differ: tests/test_host_logic.py's tolerance
        if k.endswith(".energy") or k.endswith(".table"):
            x, y = (z[k] if k.endswith(".energy") else z[k][:, 1] for z in (za, zb))
            if x.shape != y.shape or np.abs(x - y).max() >= 1e-10:
                loose[k] = "shape" if x.shape != y.shape else float(np.abs(x - y).max())
        elif k.endswith(".n_iter") and za[k] != zb[k]:
            loose[k] = [int(za[k]), int(zb[k])]
    ok = not differ and not outside_batch and not loose
    print(json.dumps({"mode": "bits", "arrays": len(za.files), "bytes": int(sum(za[k].nbytes for k in za.files)),
                      "compared_byte_for_byte": len(za.files) - len(unstable), "left_out_A_differs_from_A_prime": unstable,
                      "left_out_outside_the_batch": outside_batch, "batch_outside_tolerance": loose,
                      "result": "all equal" if ok else "DIFFERENT", "max_ulps_of_the_arrays_that_differ": differ,
                      "paths_A": infos[0]["paths"], "paths_equal_in_all_three": infos[0]["paths"] == infos[1]["paths"] == infos[2]["paths"]}))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", nargs=2, metavar="LIB")
    ap.add_argument("--time", nargs=2, metavar="LIB")
    ap.add_argument("--out", default=".")
    ap.add_argument("--limit", type=float, default=None, help="time limit of one child in seconds (default 300)")
    ap.add_argument("--child-bits")
    ap.add_argument("--child-time", action="store_true")
    a = ap.parse_args()
    if a.child_bits:
        return child_bits(a.child_bits)
    if a.child_time:
        return child_time()
    os.makedirs(a.out, exist_ok=True)
    if a.bits:
        files = [os.path.join(a.out, f"scf_bits_{name}.npz") for name in ("a", "a2", "b")]
        infos = []
        for lib, path in zip((a.bits[0], a.bits[0], a.bits[1]), files):
            infos.append(run_child(lib, ["--child-bits", path], a.limit or 300))
            if infos[-1] is None:
                return 1
            print(path, infos[-1]["arrays"], "arrays", flush=True)
        return compare_bits(files, infos)
    if a.time:
        series = {"A": [], "B": [], "A'": []}
        for rep in range(3):
            for name, lib in (("A", a.time[0]), ("B", a.time[1]), ("A'", a.time[0])):
                r = run_child(lib, ["--child-time"], a.limit or 300)
                if r is None:
                    return 1
                series[name].append(r)
                print(name, rep, json.dumps(r), flush=True)
        out = {"mode": "time", "what": "seconds of the second of two calls per cycle; medians of three processes"}
        for cycle in series["A"][0]:
            out[cycle] = {"n_iter": sorted({r[cycle]["n_iter"] for runs in series.values() for r in runs})}
            for key in SECONDS:
                runs = {name: [r[cycle][key] for r in rs] for name, rs in series.items()}
                med = {name: float(np.median(v)) for name, v in runs.items()}
                before = runs["A"] + runs["A'"]
                out[cycle][key] = {"runs": runs, "median": med, "range_of_A_and_A_prime": max(before) - min(before),
                                   "B_median_within_A_to_A_prime": abs(med["B"] - med["A"]) <= abs(med["A'"] - med["A"]),
                                   "every_B_inside_range": min(before) <= min(runs["B"]) and max(runs["B"]) <= max(before)}
        print(json.dumps(out))
        return 0
    ap.error("one of --bits and --time")


if __name__ == "__main__":
    sys.exit(main() or 0)
