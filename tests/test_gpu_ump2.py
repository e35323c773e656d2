"""GPU: unrestricted MP2 on the resident tensor (tf_mp2_uhf: tfmp2::ump2_spin_pass, mo_bra1_kernel<3>, ump2_energy_kernel, and the
general transformation block by block) against the reference program's run_unrestricted_MP2 (tests/golden/ump2_systems.npz) and the
independent NumPy UMP2 of tests/ump2_reference.py; the closed-shell limit against tf_mp2_rhf; every layout; two ranks; the input
lines of energy.run.  Every test hands the shared context back with the default layout."""
import os
import socket

import numpy as np
import pytest

import ump2_reference as ur
from conftest import R_N2, make_system, make_uhf_system
from tuna_amd import molecule as mol
from tuna_amd._lib import TunaError

pytestmark = pytest.mark.gpu

TF_EINVAL = -1
EXTRA = {"h_ccpvdz": (["H"], None, "cc-pVDZ"), "o2_triplet_ccpvtz": (["O", "O"], mol.angstrom_to_bohr(1.2075), "cc-pVTZ"),
         "n2_ccpvtz": (["N", "N"], R_N2, "cc-pVTZ")}


@pytest.fixture(scope="module")
def ump2_golden(golden):
    z = golden("ump2_systems")
    out = {}
    for key in z.files:
        tag, name = key.split("__", 1)
        out.setdefault(tag, {})[name] = z[key]
    return out


def _system(tag):
    if tag in EXTRA:
        sym, R, basis = EXTRA[tag]
        atoms = mol.make_atoms(sym, R)
        shells = mol.build_shells(atoms, basis)
        return atoms, shells, mol.expand_cartesian_aos(shells)
    atoms, shells, aos, _, _ = make_uhf_system(tag)
    return atoms, shells, aos


def _synthetic(n_sph):
    counts = mol.synthetic_counts(n_sph)
    atoms = mol.make_atoms(["AR", "AR"], 7.1)
    shells = mol.build_shells(atoms, {18: mol.even_tempered_basis(*counts)})
    return atoms, shells, mol.expand_cartesian_aos(shells)


def _reset(engine):
    engine._check(engine._L.tf_set_eri_layout(engine._ctx, -1))


def _pairs(r):
    return np.array([r["E_aa"], r["E_bb"], r["E_ab"]])


def _random_uhf(N, seed):
    """Random orthonormal C_alpha != C_beta and ascending eigenvalues with a gap at every occupation used below."""
    rng = np.random.default_rng(seed)
    Ca, Cb = (np.linalg.qr(rng.standard_normal((N, N)))[0] for _ in range(2))
    ea = np.concatenate([-np.linspace(20.0, 0.5, 45), np.linspace(0.3, 8.0, N - 45)])
    eb = np.concatenate([-np.linspace(19.0, 0.4, 45), np.linspace(0.35, 9.0, N - 45)])
    return Ca, Cb, ea, eb


@pytest.fixture(scope="module")
def n2_tz():
    atoms, shells, aos = _system("n2_ccpvtz")
    return aos, ur.dense_eri(aos, shells)


@pytest.mark.parametrize("tag", ["o2_triplet_sto3g", "o2_triplet_ccpvdz", "no_doublet_631g", "oh_doublet_ccpvdz", "li_doublet_631g",
                                 "h_ccpvdz", "o2_triplet_ccpvtz"])
def test_reference_orbitals_against_goldens(engine, ump2_golden, tag):
    g = ump2_golden[tag]
    _, _, aos = _system(tag)
    engine.set_basis(aos).build_eri(True)
    na, nb = int(g["n_alpha"]), int(g["n_beta"])
    args = (g["C_alpha"], g["C_beta"], g["eps_alpha"], g["eps_beta"], na, nb)
    r = engine.mp2_uhf(*args)
    err = np.abs(_pairs(r) - [float(g["E_aa"]), float(g["E_bb"]), float(g["E_ab"])]).max()
    print(f"\n[{tag}] N = {engine.N}: E_aa {r['E_aa']:.12f} E_bb {r['E_bb']:.12f} E_ab {r['E_ab']:.12f}, max err {err:.2e}")
    assert err < 1e-10
    assert r["E_MP2"] == r["E_SS"] + r["E_OS"] and r["E_OS"] == r["E_ab"]
    if tag == "h_ccpvdz":
        assert r["E_aa"] == 0.0 and r["E_bb"] == 0.0 and r["E_ab"] == 0.0
    if na == 1:
        assert abs(r["E_aa"]) < 1e-14
    if nb == 1:
        assert abs(r["E_bb"]) < 1e-14
    for kf in (2, 3):
        if f"fc{kf}_E_aa" not in g:
            continue
        fa, fb = ur.frozen_split(kf)
        r = engine.mp2_uhf(*args, n_frozen_alpha=fa, n_frozen_beta=fb)
        want = [float(g[f"fc{kf}_E_aa"]), float(g[f"fc{kf}_E_bb"]), float(g[f"fc{kf}_E_ab"])]
        assert np.abs(_pairs(r) - want).max() < 1e-10, (kf, _pairs(r), want)


WIDTHS = [(1, 0), (2, 1), (9, 7), (16, 15), (17, 16), (20, 18), (32, 30), (33, 31), (40, 38)]


def test_widths_against_the_independent_checker(engine, n2_tz):
    """N2/cc-pVTZ with random C_alpha != C_beta: one and two MFMA column tiles, the vector-ALU columns (17-20), the stacked bra above 32
    (mo_bra1_kernel<3>), 32 | 33 (the general path), and an empty beta block."""
    aos, E = n2_tz
    engine.set_basis(aos).build_eri(True)
    N = engine.N
    Ca, Cb, ea, eb = _random_uhf(N, 60)
    worst = 0.0
    for na, nb in WIDTHS:
        got = _pairs(engine.mp2_uhf(Ca, Cb, ea, eb, na, nb))
        want = np.array(ur.pair_energies(E, Ca, Cb, ea, eb, na, nb))
        err = float(np.abs(got - want).max())
        worst = max(worst, err)
        assert err < 1e-10, ((na, nb), got, want)
        if nb == 0:
            assert got[1] == 0.0 and got[2] == 0.0
    print(f"\n[widths] N2/cc-pVTZ, worst |dE| {worst:.2e} over {WIDTHS}")


@pytest.fixture(scope="module")
def synth400(engine):
    """synth-400 (the bench workload) with its converged RHF orbitals, as bench.scf_on_workload runs the cycle."""
    atoms, shells, aos = _synthetic(400)
    engine.set_basis(aos).build_eri(True)
    xyz, chg = [a.origin for a in atoms], [float(a.charge) for a in atoms]
    nocc = 18
    S, T, V, _, _ = engine.one_electron(xyz, chg, [0, 0, 0.5 * atoms[-1].origin[2]])
    X, _, _ = engine.orthogonaliser(S)
    _, C0 = engine.diagonalise(T + V, X)
    P0 = 2.0 * C0[:, :nocc] @ C0[:, :nocc].T
    P0 = 0.5 * (P0 + P0.T)
    nao = [sum(s.n_sph for s in shells if s.atom == a) for a in range(len(atoms))]
    args = (S, T, V, P0, float(np.sum(P0 * (T + V))), nocc, mol.nuclear_repulsion(atoms))
    try:
        r = engine.scf_rhf(*args, X=X, conv="tight", damping="none", n_atom_ao=nao, max_iter=100)
    except TunaError:
        r = engine.scf_rhf(*args, X=X, conv="tight", damping="dynamic", n_atom_ao=nao, max_iter=200)
    return aos, r["C"], r["epsilons"], nocc


def _closed_shell_check(engine, C, eps, o):
    rr = engine.mp2_rhf(C, eps, o)
    ru = engine.mp2_uhf(C, C, eps, eps, o, o)
    rel = lambda a, b: abs(a - b) / max(1e-300, abs(b))          # noqa: E731
    assert rel(ru["E_ab"], rr["E_OS"]) < 1e-11, (ru, rr)
    assert rel(ru["E_aa"], 0.5 * rr["E_SS"]) < 1e-11 and rel(ru["E_bb"], 0.5 * rr["E_SS"]) < 1e-11, (ru, rr)
    return rr, ru


def test_closed_shell_limit_and_spin_swap(engine, ump2_golden, n2_tz, synth400):
    g = ump2_golden["n2_ccpvtz"]
    engine.set_basis(n2_tz[0]).build_eri(True)
    _closed_shell_check(engine, g["C_alpha"], g["eps_alpha"], 7)
    Ca, Cb, ea, eb = _random_uhf(engine.N, 61)
    r1 = engine.mp2_uhf(Ca, Cb, ea, eb, 9, 7)
    r2 = engine.mp2_uhf(Cb, Ca, eb, ea, 7, 9)
    assert abs(r1["E_aa"] - r2["E_bb"]) < 1e-13 and abs(r1["E_bb"] - r2["E_aa"]) < 1e-13
    assert abs(r1["E_ab"] - r2["E_ab"]) <= 1e-12 * abs(r1["E_ab"])
    aos, C, eps, nocc = synth400
    engine.set_basis(aos).build_eri(True)
    rr, ru = _closed_shell_check(engine, C, eps, nocc)
    print(f"\n[synth-400] RMP2 {rr['E_MP2']:.12f} UMP2 {ru['E_MP2']:.12f} ({ru['seconds'] * 1e3:.1f} ms vs {rr['seconds'] * 1e3:.1f} ms)")


def test_layouts_agree(engine, n2_tz):
    """rows and tiles (the general transformation block by block) equal packed (the spin-blocked route) on N2/cc-pVTZ and synth-200."""
    cases = [(n2_tz[0], 60, (9, 7)), (_synthetic(200)[2], 200, (19, 17))]
    try:
        for aos, N, (na, nb) in cases:
            Ca, Cb, ea, eb = _random_uhf(N, N)
            e = {}
            for layout in ("packed", "tiles", "rows"):
                engine.set_basis(aos).build_eri(True, layout=layout)
                assert engine.eri_storage()["layout"] == layout and engine.N == N
                e[layout] = _pairs(engine.mp2_uhf(Ca, Cb, ea, eb, na, nb))
            for lt in ("tiles", "rows"):
                assert np.all(np.abs(e[lt] - e["packed"]) <= 1e-12 * np.abs(e["packed"])), (N, lt, e[lt], e["packed"])
    finally:
        _reset(engine)
    engine.set_basis(n2_tz[0]).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed"


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_ump2(rank, world, port, ret):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from tuna_amd import distributed as tdist
        from tuna_amd.engine import Engine
        gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "ump2_systems.npz"))
        g = {k.split("__", 1)[1]: gold[k] for k in gold.files if k.startswith("o2_triplet_ccpvdz__")}
        _, _, aos, na, nb = make_uhf_system("o2_triplet_ccpvdz")
        with Engine(0, rank, world) as eng:
            eng.set_basis(aos).build_eri(True)
            try:
                eng.mp2_uhf(g["C_alpha"], g["C_beta"], g["eps_alpha"], g["eps_beta"], na, nb)
                refused = False
            except Exception as e:                                   # partial sums must not be returned as the result
                refused = "tf_set_allreduce" in str(e)
            tdist.attach_allreduce(eng)
            r = eng.mp2_uhf(g["C_alpha"], g["C_beta"], g["eps_alpha"], g["eps_beta"], na, nb)
            ret[rank] = (refused, r["E_aa"], r["E_bb"], r["E_ab"])
    finally:
        dist.destroy_process_group()


def test_sharded_tensor_equals_one_rank(engine, ump2_golden):
    import torch.multiprocessing as mp
    world = 2
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_rank_ump2, args=(world, _free_port(), ret), nprocs=world, join=True)
        res = dict(ret)
    assert set(res) == {0, 1}
    g = ump2_golden["o2_triplet_ccpvdz"]
    _, _, aos, na, nb = make_uhf_system("o2_triplet_ccpvdz")
    engine.set_basis(aos).build_eri(True)
    one = _pairs(engine.mp2_uhf(g["C_alpha"], g["C_beta"], g["eps_alpha"], g["eps_beta"], na, nb))
    for rank, (refused, *e) in res.items():
        assert refused
        assert np.all(np.abs(np.array(e) - one) <= 1e-12 * np.abs(one)), (rank, e, one)


def test_repeatable_and_refusals(engine, ump2_golden, mp2_golden):
    from tuna_amd.engine import Engine
    g = ump2_golden["o2_triplet_ccpvdz"]
    _, _, aos, na, nb = make_uhf_system("o2_triplet_ccpvdz")
    engine.set_basis(aos).build_eri(True)
    args = (g["C_alpha"], g["C_beta"], g["eps_alpha"], g["eps_beta"], na, nb)
    a, b = engine.mp2_uhf(*args), engine.mp2_uhf(*args)
    assert all(a[k] == b[k] for k in ("E_aa", "E_bb", "E_ab"))
    L, ctx, N = engine._L, engine._ctx, engine.N
    Ca, Cb, ea, eb = (np.ascontiguousarray(x, dtype=np.float64) for x in args[:4])
    out = (np.ctypeslib.ctypes.c_double * 3)()
    p = lambda x: x.ctypes.data_as(np.ctypeslib.ctypes.c_void_p)   # noqa: E731
    bad = [(na, nb, -1, 0, p(Ca), p(Cb), p(ea), p(eb)), (na, nb, 0, -1, p(Ca), p(Cb), p(ea), p(eb)),
           (na, nb, na + 1, 0, p(Ca), p(Cb), p(ea), p(eb)), (na, nb, 0, nb + 1, p(Ca), p(Cb), p(ea), p(eb)),
           (N, nb, 0, 0, p(Ca), p(Cb), p(ea), p(eb)), (na, N, 0, 0, p(Ca), p(Cb), p(ea), p(eb)),
           (na, nb, 0, 0, None, p(Cb), p(ea), p(eb)), (na, nb, 0, 0, p(Ca), None, p(ea), p(eb)),
           (na, nb, 0, 0, p(Ca), p(Cb), None, p(eb)), (na, nb, 0, 0, p(Ca), p(Cb), p(ea), None)]
    for args_c in bad:
        assert L.tf_mp2_uhf(ctx, *args_c, out, None) == TF_EINVAL, args_c
    assert L.tf_mp2_uhf(ctx, na, nb, 0, 0, p(Ca), p(Cb), p(ea), p(eb), None, None) == TF_EINVAL
    with Engine(0) as fresh:                                          # no tensor yet
        fresh.set_basis(aos)
        assert fresh._L.tf_mp2_uhf(fresh._ctx, na, nb, 0, 0, p(Ca), p(Cb), p(ea), p(eb), out, None) == TF_EINVAL
    # the context stays usable: RMP2 gives its pinned value afterwards
    m = mp2_golden["n2_ccpvdz"]
    _, _, aos2, nocc = make_system("n2_ccpvdz")
    engine.set_basis(aos2).build_eri(True)
    r = engine.mp2_rhf(m["C"], m["eps"], nocc)
    assert abs(r["E_OS"] - float(m["E_OS"])) < 1e-10 and abs(r["E_SS"] - float(m["E_SS"])) < 1e-10


def test_input_lines(engine, ump2_golden):
    from tuna_amd.energy import run
    lines = []
    o2tz, no, n2, o2dz = (ump2_golden[t] for t in ("o2_triplet_ccpvtz", "no_doublet_631g", "n2_ccpvtz", "o2_triplet_ccpvdz"))
    tot = lambda g: float(g["E_UHF"]) + float(g["E_aa"]) + float(g["E_bb"]) + float(g["E_ab"])   # noqa: E731
    cases = [("SPE : O O 1.2075 : MP2 CC-PVTZ : ML 3 EXTREME", tot(o2tz)),
             ("SPE : N O 1.1508 : UMP2 6-31G : ML 2 EXTREME", tot(no)),
             ("SPE : N N 1.0977 : SCS-MP2 CC-PVTZ : EXTREME", float(n2["E_UHF"]) + float(n2["scs_E_MP2"])),
             ("SPE : O O 1.2075 : USCS-MP2 CC-PVDZ : ML 3 EXTREME", float(o2dz["E_UHF"]) + float(o2dz["scs_E_MP2"])),
             ("SPE : O O 1.2075 : USCS-MP2 CC-PVDZ : ML 3 EXTREME SSS 0.5 OSS 1.1",
              float(o2dz["E_UHF"]) + 0.5 * (float(o2dz["E_aa"]) + float(o2dz["E_bb"])) + 1.1 * float(o2dz["E_ab"])),
             ("SPE : O O 1.2075 : MP2 CC-PVDZ : ML 3 EXTREME SSS 0.5 OSS 1.1", tot(o2dz))]
    for k, (line, want) in enumerate(cases):
        log = []
        out = run(line, silent=(k > 0), engine=engine, log=log.append)
        print(f"\n[{line}] E = {out.energy:.10f} (golden {want:.10f}, d {out.energy - want:.1e})")
        assert abs(out.energy - want) < 1e-8, (line, out.energy, want)
        assert out.correlation_energy_mp2 == out.mp2["E_MP2"]
        lines += log
    text = "\n".join(lines)
    for s in ("Unrestricted Hartree-Fock energy:", "Energy from alpha-alpha pairs:", "Energy from beta-beta pairs:",
              "Energy from alpha-beta pairs:", "Same spin contribution:", "Opposite spin contribution:", "MP2 correlation energy:",
              "Final single point energy:"):
        assert s in text, s
    log = []
    run("SPE : N N 1.0977 : SCS-MP2 STO-3G", silent=False, engine=engine, log=log.append)
    assert any("Same-spin scaling: 0.333" in s for s in log) and any("Opposite-spin scaling: 1.200" in s for s in log)
    with pytest.raises(TunaError, match="guess-orbital rotation"):
        run("SPE : N N 1.0977 : UMP2 STO-3G", engine=engine)
