"""GPU: the AO->MO transformation and RMP2 (tf_mp2.hip.h, mo_transform_device) at the sizes and on the layouts where their paths switch:
the first quarter without C3 in LDS (mo_q1_kernel<NT, false>), the bra kernel above 64 KB of LDS, the expanded-block path over several
slabs of rows, the tiles and rows layouts, frozen core -- and the RMP2 energy bench.py prints for synth-400.

No dense tensor fits at N >= 400 (205 GB), so the reference is a Coulomb contraction: for bra columns a_p, b_q and
D = (a_p b_q^T + b_q a_p^T) / 2, J(D)[l s] = sum_mn (mn|ls) a_mp b_nq, hence C3^T J(D) C4 = out[p, q, :, :] exactly.  tf_fock_jk (always
the full task list) is pinned element by element at N = 400 (test_gpu_parity.py) and is re-checked here at N = 520.
Every test hands the shared context back with the default layout."""
import numpy as np
import pytest

from test_gpu_scf_large import E_MP2_SYNTH400, E_MP2_SYNTH400_TOL
from tuna_amd import molecule as mol
from tuna_amd.engine import Engine

pytestmark = pytest.mark.gpu


def _synthetic(n_sph):
    counts = mol.synthetic_counts(n_sph)
    atoms = mol.make_atoms(["AR", "AR"], 7.1)
    shells = mol.build_shells(atoms, {18: mol.even_tempered_basis(*counts)})
    return atoms, shells, mol.expand_cartesian_aos(shells)


def _reset(engine):
    engine._check(engine._L.tf_set_eri_layout(engine._ctx, -1))


def _orthonormal(rng, N, n):
    return np.linalg.qr(rng.standard_normal((N, n)))[0] if n <= N else rng.standard_normal((N, n)) / np.sqrt(N)


# ---- a mirror of the path selection of mo_transform_device (run()) and tfmp2::transform_q1 / transform ------------------------------------
def _geometry(eng):
    """(N, AOs per parity class, stored rows per class): the class of a spherical AO is that of the first Cartesian component of its row of
    the spherical matrix, as bench.mp2_leg counts it"""
    U, lmn = eng.sph_matrix(), np.asarray(eng.aos.lmn)
    first = np.argmax(np.abs(U) > 0, axis=1)
    cls = (lmn[first, 0] & 1) | ((lmn[first, 1] & 1) << 1)
    hi, lo = np.tril_indices(U.shape[0])
    return U.shape[0], [int(x) for x in np.bincount(cls, minlength=4)], [int(x) for x in np.bincount(cls[hi] ^ cls[lo], minlength=4)]


def _q1_kernel(N, csize, n3, nx=True):
    nblk = sum((s + 15) // 16 for s in csize)
    n3r = (n3 + 1) & ~1
    lds_tab = 4 * N * 8 + 4 * 32 + (4 * nblk + 4) * 4              # segment tables | Q1Row headers | block starts + counter
    blds = lds_tab + N * n3r * 8 <= 80 << 10
    if blds and 16 < n3 <= 20 and nx:
        return f"q1 NX{n3 - 16}"
    return f"q1 <{(n3 + 15) // 16},{'true' if blds else 'false'}>"


def _bra_kernel(N, n1):
    lds1 = N * ((n1 + 1) & ~1) * 8 + 4 * N
    return f"bra <{1 if n1 <= 16 else 2}>" + (" >64KB" if lds1 > 64 << 10 else "")


def _paths(geo, shape, layout="packed", q1=True, nx=True, same_pairs=False):
    """the kernels / paths a transformation of `shape` = (n1, n2, n3, n4) takes (the q1 work pool assumed to fit)"""
    N, csize, rows_c = geo
    n_rows = N * (N + 1) // 2
    packed = layout != "rows"
    out = set()
    for a, c in ([(0, 2)] if not packed or same_pairs else [(0, 2), (2, 0)]):     # packed: run(0,1,2,3) and run(2,3,0,1)
        na, nc = shape[a], shape[c]
        if layout == "packed" and q1 and nc <= 32 and na <= 32 and N * ((na + 1) & ~1) * 8 + 4 * N <= 150 << 10:
            out |= {_q1_kernel(N, csize, nc, nx), _bra_kernel(N, na)}
            continue
        slab = max(1, min(n_rows, (2048 << 20) // (nc * N * 8)))
        if packed:
            max_rs = max((sum(csize[x] * max(1, csize[x ^ cc]) for x in range(4)) + 1) & ~1 for cc in range(4))
            slab = max(1, min(slab, 65535, (2048 << 20) // (max_rs * 8)))
            n_slabs = max(-(-r // slab) for r in rows_c)
        else:
            n_slabs = -(-n_rows // slab)
        out.add("block, several slabs" if n_slabs > 1 else "block, one slab")
    return out


EVERY_PATH = {"q1 <1,true>", "q1 <2,true>", "q1 NX1", "q1 NX2", "q1 NX3", "q1 NX4", "q1 <1,false>", "q1 <2,false>",
              "bra <1>", "bra <1> >64KB", "bra <2>", "bra <2> >64KB", "block, several slabs"}

# (n1, n2, n3, n4), TF_Q1_NX, the paths by the mirror.  Checked once on MI355X against a kernel trace of the shape tests: the dispatched
# instantiations, their dynamic LDS (77360 bytes for NX4 at N = 400, 65600 / 72000 / 104000 for the bra kernel, 68640 at N = 520) and 16
# unpack_own_rows_blocked_kernel launches per block-path transformation of (1, 2, 33, 4) -- 5 + 4 + 4 + 3 slabs -- are the mirror's.
SHAPES_400 = [((20, 1, 20, 3), None, {"q1 NX4", "bra <2> >64KB"}),
              ((2, 3, 21, 5), None, {"q1 <2,false>", "bra <1>", "q1 <1,true>", "bra <2> >64KB"}),
              ((32, 1, 32, 2), None, {"q1 <2,false>", "bra <2> >64KB"}),
              ((1, 2, 33, 4), None, {"block, several slabs"}),
              ((19, 1, 17, 2), None, {"q1 NX1", "bra <2> >64KB", "q1 NX3", "bra <2>"}),
              ((17, 2, 18, 3), "0", {"q1 <2,true>", "bra <2>"})]
SHAPE_520 = ((2, 3, 16, 5), {"q1 <1,false>", "bra <1>", "q1 <1,true>", "bra <1> >64KB"})
BENCH_PATHS = {"q1 NX2", "bra <2>"}                       # the bench leg: (ia|jb), 18 occupied orbitals, one transformation
BENCH_PATHS_NO_Q1 = {"block, several slabs"}             # the same under TF_MO_Q1=0 (and on the tiles layout)


def _j_slices(eng, A, B, C3, C4, pairs, batch=64):
    """[len(pairs), n3, n4]: out[p, q, :, :] = C3^T J(D_pq) C4 for the bra columns (p of A, q of B), densities batched per call"""
    res = []
    for s in range(0, len(pairs), batch):
        D = np.stack([np.outer(A[:, p], B[:, q]) + np.outer(B[:, q], A[:, p]) for p, q in pairs[s:s + batch]]) * 0.5
        J, _ = eng.fock_jk(D)
        res.append(np.matmul(C3.T, np.matmul(J, C4)))
    return np.concatenate(res)


def _mp2_numpy(g, eps_o, eps_v):
    """(E_OS, E_SS) of g[i, a, j, b] = (ia|jb) (tuna_mp.py:882-890)"""
    D = eps_o[:, None, None, None] - eps_v[None, :, None, None] + eps_o[None, None, :, None] - eps_v[None, None, None, :]
    return float(np.sum(g * g / D)), float(np.sum(g * (g - g.transpose(0, 3, 2, 1)) / D))


@pytest.fixture(scope="module")
def bench_orbitals(engine):
    """Converged orbitals of the bench leg: synth-400, native RHF exactly as bench.scf_on_workload runs it (core guess from tf_diagonalise,
    TIGHT, undamped first, dynamic damping if that does not converge)."""
    from tuna_amd._lib import TunaError
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


def test_every_kernel_variant_is_reached(engine):
    """The mirror of the selection formulas over the shapes of this file: every instantiation of mo_q1_kernel / mo_bra1_kernel, the
    bra kernel on both sides of 64 KB of LDS and the block path over several slabs."""
    reached = set()
    for n, shapes in ((400, SHAPES_400), (520, [(SHAPE_520[0], None, SHAPE_520[1])])):
        engine.set_basis(_synthetic(n)[2])
        geo = _geometry(engine)
        assert geo[0] == n and sum(geo[2]) == n * (n + 1) // 2
        for shape, nx, want in shapes:
            got = _paths(geo, shape, nx=nx != "0")
            assert got == want, (n, shape, got)
            reached |= got
        if n == 400:
            o, v = 18, n - 18
            assert _paths(geo, (o, v, o, v), same_pairs=True) == BENCH_PATHS
            assert _paths(geo, (o, v, o, v), same_pairs=True, q1=False) == BENCH_PATHS_NO_Q1
            assert _paths(geo, (o, v, o, v), layout="tiles", same_pairs=True) == BENCH_PATHS_NO_Q1
            reached |= BENCH_PATHS | BENCH_PATHS_NO_Q1
    assert reached == EVERY_PATH, EVERY_PATH - reached


def test_bench_leg_ovov_against_coulomb_contractions_and_numpy_energies(engine, bench_orbitals, monkeypatch):
    """synth-400, the converged orbitals of the bench leg: (ia|jb) rows g[i, a, :, :] for every i and 16 virtuals each (first, last, both
    sides of the 16-, 32-, 64- and 128-column boundaries, six at random) against J contractions; E_OS / E_SS of tf_mp2_rhf on the q1 path and
    on the block path (TF_MO_Q1=0: several slabs per class) against NumPy on the full g; frozen core 10 and 17 against slices of g."""
    aos, C, eps, o = bench_orbitals
    engine.set_basis(aos).build_eri(True)
    N = engine.N
    v = N - o
    Co, Cv = C[:, :o], C[:, o:]
    monkeypatch.delenv("TF_MO_Q1", raising=False)
    g = engine.ao_to_mo(Co, Cv, Co, Cv)
    rng = np.random.default_rng(400)
    fixed = [0, 15, 16, 31, 32, 63, 64, 127, 128, v - 1]
    pairs = []
    for i in range(o):
        extra = rng.choice(np.setdiff1d(np.arange(v), fixed), size=6, replace=False)
        pairs += [(i, int(a)) for a in fixed + sorted(extra.tolist())]
    ref = _j_slices(engine, Co, Cv, Co, Cv, pairs)
    got = np.stack([g[i, a] for i, a in pairs])
    err = float(np.abs(got - ref).max())
    scale = max(1.0, float(np.abs(ref).max()))
    print(f"\n[synth-400 ovov] {len(pairs)} rows, max|g - J ref| {err:.2e} (scale {scale:.3g})")
    assert err <= 1e-11 * scale
    e_os, e_ss = _mp2_numpy(g, eps[:o], eps[o:])
    r1 = engine.mp2_rhf(C, eps, o)
    monkeypatch.setenv("TF_MO_Q1", "0")
    r0 = engine.mp2_rhf(C, eps, o)
    monkeypatch.delenv("TF_MO_Q1", raising=False)
    dev = {k: max(abs(r[k] - ref_e) for r in (r1, r0)) for k, ref_e in (("E_OS", e_os), ("E_SS", e_ss))}
    print(f"[synth-400 MP2] E_OS {e_os:.12f} E_SS {e_ss:.12f} E_MP2 {e_os + e_ss:.12f}; q1 {r1['E_MP2']:.12f}, blocks {r0['E_MP2']:.12f}; "
          f"max dev {dev}")
    assert dev["E_OS"] <= 1e-10 and dev["E_SS"] <= 1e-10, dev
    for nf in (10, 17):
        rf = engine.mp2_rhf(C, eps, o, nf)
        f_os, f_ss = _mp2_numpy(g[nf:, :, nf:, :], eps[nf:o], eps[o:])
        print(f"[synth-400 MP2, {nf} frozen] dE_OS {abs(rf['E_OS'] - f_os):.2e} dE_SS {abs(rf['E_SS'] - f_ss):.2e}")
        assert abs(rf["E_OS"] - f_os) <= 1e-10 and abs(rf["E_SS"] - f_ss) <= 1e-10, (nf, rf, f_os, f_ss)
        assert abs(rf["E_MP2"] - r1["E_MP2"]) > 1e-6                   # (the frozen orbitals did leave)


def test_bench_scf_on_workload_prints_the_pinned_mp2_energy():
    """bench.scf_on_workload on a fresh context: the E_MP2_Eh of the bench line is the pinned synth-400 RMP2 energy."""
    import bench
    with Engine(0) as eng:
        atoms, shells, aos, nocc, desc = bench.build_workload("synth-400")
        eng.set_basis(aos).build_eri(True)
        res = bench.scf_on_workload(eng, atoms, shells, nocc, desc)
    assert "error" not in res, res
    e = res["mp2"]["E_MP2_Eh"]
    print(f"\n[bench synth-400] E_MP2_Eh {e:.12f} (pin {E_MP2_SYNTH400:.12f}, d {abs(e - E_MP2_SYNTH400):.2e}), damping {res['damping']}")
    assert abs(e - E_MP2_SYNTH400) <= E_MP2_SYNTH400_TOL


@pytest.mark.parametrize("shape,nx,want", SHAPES_400, ids=[f"{s[0]}x{s[1]}x{s[2]}x{s[3]}" + ("-nx0" if nx else "") for s, nx, _ in SHAPES_400])
def test_shapes_at_400_against_coulomb_contractions(engine, shape, nx, want, monkeypatch):
    """synth-400, four different orthonormal coefficient blocks: every slice out[p, q, :, :] against C3^T J(D_pq) C4."""
    aos = _synthetic(400)[2]
    engine.set_basis(aos).build_eri(True)
    N = engine.N
    assert _paths(_geometry(engine), shape, nx=nx != "0") == want
    rng = np.random.default_rng(sum(shape))
    Cs = [_orthonormal(rng, N, n) for n in shape]
    monkeypatch.delenv("TF_MO_Q1", raising=False)
    if nx is None:
        monkeypatch.delenv("TF_Q1_NX", raising=False)
    else:
        monkeypatch.setenv("TF_Q1_NX", nx)
    out = engine.ao_to_mo(*Cs)
    pairs = [(p, q) for p in range(shape[0]) for q in range(shape[1])]
    ref = _j_slices(engine, Cs[0], Cs[1], Cs[2], Cs[3], pairs).reshape(shape)
    err, scale = float(np.abs(out - ref).max()), max(1.0, float(np.abs(ref).max()))
    print(f"\n[synth-400 {shape}] max|out - J ref| {err:.2e} (scale {scale:.3g})")
    assert err <= 1e-11 * scale


def test_shape_at_520_against_coulomb_contractions():
    """synth-520 (the first size where 16 columns of C3 do not fit LDS beside the row tables: mo_q1_kernel<1, false>): J re-checked element by
    element against sampled tensor rows first, then out[p, q, :, :] against C3^T J(D_pq) C4.  A context of its own: the tensor and the q1
    work pool of this size are released at the end."""
    shape, want = SHAPE_520
    with Engine(0) as eng:
        eng.set_basis(_synthetic(520)[2]).build_eri(True)
        N = eng.N
        assert N == 520 and eng.eri_storage()["layout"] == "packed"
        assert _paths(_geometry(eng), shape) == want
        rng = np.random.default_rng(520)
        A = rng.standard_normal((N, N))
        P = A + A.T
        J, _ = eng.fock_jk(P)
        kk, ll = (x.reshape(-1).astype(np.int32) for x in np.meshgrid(np.arange(N), np.arange(N), indexing="ij"))
        sJ = np.abs(J).max()
        for a, b in [(0, 0), (N - 1, N - 1), (N - 1, 0), (259, 260), (260, 259), (519, 260), (17, 403), (333, 101)]:
            M = eng.sample_eri(np.stack([np.full(N * N, a, np.int32), np.full(N * N, b, np.int32), kk, ll], axis=1)).reshape(N, N)
            assert abs(J[a, b] - np.sum(M * P)) < 1e-10 * sJ, (a, b)
        Cs = [_orthonormal(rng, N, n) for n in shape]
        out = eng.ao_to_mo(*Cs)
        pairs = [(p, q) for p in range(shape[0]) for q in range(shape[1])]
        ref = _j_slices(eng, Cs[0], Cs[1], Cs[2], Cs[3], pairs).reshape(shape)
    err, scale = float(np.abs(out - ref).max()), max(1.0, float(np.abs(ref).max()))
    print(f"\n[synth-520 {shape}] max|out - J ref| {err:.2e} (scale {scale:.3g})")
    assert err <= 1e-11 * scale


def test_tiles_and_rows_at_200_against_packed(engine):
    """synth-200 on all three layouts: a q1-width shape and a wide ket (240 columns: the block path over several slabs of rows on each
    layout, by the mirror) against the packed result and C3^T J C4; the RMP2 energy of 18 occupied orbitals on each layout."""
    aos = _synthetic(200)[2]
    rng = np.random.default_rng(200)
    N = 200
    shapes = [(4, 6, 18, 7), (2, 3, 240, 4)]
    Cs = [[_orthonormal(rng, N, n) for n in s] for s in shapes]
    Q = np.linalg.qr(rng.standard_normal((N, N)))[0]
    eps = np.concatenate([-np.linspace(3.0, 0.5, 18), np.linspace(0.4, 6.0, N - 18)])
    out, e = {}, {}
    try:
        for layout in ("packed", "tiles", "rows"):
            engine.set_basis(aos).build_eri(True, layout=layout)
            assert engine.eri_storage()["layout"] == layout and engine.N == N
            geo = _geometry(engine)
            assert "block, several slabs" in _paths(geo, shapes[1], layout=layout)
            out[layout] = [engine.ao_to_mo(*c) for c in Cs]
            e[layout] = engine.mp2_rhf(Q, eps, 18)
            if layout == "packed":
                refs = []
                for s, c in zip(shapes, Cs):
                    pairs = [(p, q) for p in range(s[0]) for q in range(s[1])]
                    refs.append(_j_slices(engine, c[0], c[1], c[2], c[3], pairs).reshape(s))
    finally:
        _reset(engine)
    for k, s in enumerate(shapes):
        scale = max(1.0, float(np.abs(refs[k]).max()))
        err = float(np.abs(out["packed"][k] - refs[k]).max())
        lay = {lt: float(np.abs(out[lt][k] - out["packed"][k]).max()) for lt in ("tiles", "rows")}
        print(f"\n[synth-200 {s}] packed vs J ref {err:.2e}, layouts vs packed {lay} (scale {scale:.3g})")
        assert err <= 1e-11 * scale
        assert max(lay.values()) <= 1e-12 * scale, lay
    for lt in ("tiles", "rows"):
        for k in ("E_OS", "E_SS"):
            assert abs(e[lt][k] - e["packed"][k]) <= 1e-12 * max(1.0, abs(e["packed"][k])), (lt, e[lt], e["packed"])


def test_tiles_at_400_against_packed(engine, bench_orbitals):
    """synth-400, the bench leg's orbitals on the tiles layout (the block path over several slabs, unpack_own_rows_blocked_tiles_kernel):
    the full ovov tensor and both RMP2 components against the packed layout."""
    aos, C, eps, o = bench_orbitals
    Co, Cv = C[:, :o], C[:, o:]
    try:
        engine.set_basis(aos).build_eri(True, layout="packed")
        gp, ep = engine.ao_to_mo(Co, Cv, Co, Cv), engine.mp2_rhf(C, eps, o)
        engine.build_eri(True, layout="tiles")
        assert engine.eri_storage()["layout"] == "tiles"
        gt, et = engine.ao_to_mo(Co, Cv, Co, Cv), engine.mp2_rhf(C, eps, o)
    finally:
        _reset(engine)
    scale = max(1.0, float(np.abs(gp).max()))
    err = float(np.abs(gt - gp).max())
    de = {k: abs(et[k] - ep[k]) for k in ("E_OS", "E_SS")}
    print(f"\n[synth-400 tiles vs packed] max|dg| {err:.2e} (scale {scale:.3g}), dE {de}")
    assert err <= 1e-12 * scale
    assert de["E_OS"] <= 1e-12 * max(1.0, abs(ep["E_OS"])) and de["E_SS"] <= 1e-12 * max(1.0, abs(ep["E_SS"])), de
