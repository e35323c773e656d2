"""GPU: the particle-particle ladder kernel of MP3 (tfmp3::mp3_ladder_kernel, through tf_mp3_ladder_probe) element by element, and every
MP3 term of tf_mp3_rhf against NumPy, at the sizes where the kernel's loops run more than once: synth-200 (one block group, the second
block of a wave, three 32-column passes), synth-400 (two block groups, partial last blocks, (ab|ij) in 48 slices) and synth-520 (three
groups).

No dense tensor fits at N >= 400, so every reference is built from quantities the tensor itself pins:
  * tensor planes (mu la|nu si) for fixed (mu, nu) or (la, si) from tf_sample_eri;
  * Z[T][mu][nu] = sum (mu la|nu si) T[la][si] = K[T^T][mu][nu] with K the reference string "ilkj,kl->ij" of tf_fock_jk, whose
    general-density (two-pass) build is itself compared with sampled planes here;
  * the MO blocks of tests/mp3_reference.py: terms_from_blocks from tf_ao_to_mo ((ia|jb), pinned row by row at synth-400 by
    test_gpu_mp2_large.py) and from Coulomb matrices ((ij|ab), (ki|lj): symmetric J, pinned element by element by test_gpu_parity.py).
The probe returns Zh, the contraction with the stored triangle; Z[T] = Zh[T] + Zh[T^T]^T (tests/test_mp3_reference.py).
Every test hands the shared context back with the default layout."""
import time

import numpy as np
import pytest

import mp3_reference as mr
from test_gpu_mp2_large import _geometry, _reset, _synthetic, bench_orbitals  # noqa: F401  (bench_orbitals: a fixture)
from test_gpu_mp3 import _random_orbitals, _system
from tuna_amd.engine import Engine

pytestmark = pytest.mark.gpu

TFL_W = 64                                    # pairs of a batch of the ladder kernel (tf_mp3.hip.h)
TFL_BLOCKS_PER_GROUP = 16                     # TFL_THREADS / 64 waves x TFL_MB blocks


# ---- mirrors of the library's formulas -------------------------------------------------------------------------------------------------
def _ladder_geometry(csize):
    """what mp3_ladder_kernel's loops do for parity classes of these sizes: 16-row blocks, block groups (blockIdx.y), whether a wave
    reaches its second block (q == 1 of TFL_MB: block 8 .. 15 of a group), passes of the 32-column loops over the widest class, rows of
    the last block of each class"""
    nblk = sum((s + 15) // 16 for s in csize)
    return {"nblk": nblk, "groups": -(-nblk // TFL_BLOCKS_PER_GROUP), "second_block": nblk > 8, "passes": -(-max(csize) // 32),
            "last_rows": sorted((s - 1) % 16 + 1 for s in csize if s)}


def _abij_slices(N, v):
    """slices of the first virtual index in which tf_mp3_rhf makes (ab|ij), v virtual orbitals"""
    nc = max(1, min(v, (512 << 20) // (N * N * v)))
    return [min(nc, v - a0) for a0 in range(0, v, nc)]


def _classes(eng):
    """parity class of every AO (the rule of _geometry and of tf_build_eri)"""
    U, lmn = eng.sph_matrix(), np.asarray(eng.aos.lmn)
    first = np.argmax(np.abs(U) > 0, axis=1)
    return (lmn[first, 0] & 1) | ((lmn[first, 1] & 1) << 1)


def _picks(N, seed):
    """24 output elements: the fixed ones of test_fock_rows_at_the_benched_size_against_sampled_tensor_rows and 16 at random"""
    rng = np.random.default_rng(seed)
    picks = [(0, 0), (N - 1, N - 1), (N - 1, 0), (0, N - 1), (N // 2, N // 2 - 1), (199, 200), (200, 199), (399, 200)]
    while len(picks) < 24:
        picks.append(tuple(int(x) for x in rng.integers(0, N, size=2)))
    return picks


def _grid(N):
    kk, ll = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    return kk.reshape(-1).astype(np.int32), ll.reshape(-1).astype(np.int32)


def _plane(eng, order, a, b):
    """[N, N] plane of the tensor over (k, l) with two indices fixed; order names the quadruple, e.g. "akbl" = (a k|b l)"""
    N = eng.N
    kk, ll = _grid(N)
    col = {"a": np.full(N * N, a, np.int32), "b": np.full(N * N, b, np.int32), "k": kk, "l": ll}
    return eng.sample_eri(np.stack([col[c] for c in order], axis=1)).reshape(N, N)


def _Z_from_probe(eng, T):
    """Z[T] = Zh[T] + Zh[T^T]^T, both halves from the ladder kernel"""
    T = np.asarray(T)
    Zh = eng.mp3_ladder_probe(T)
    ZhT = eng.mp3_ladder_probe(np.ascontiguousarray(np.swapaxes(T, -1, -2)))
    return Zh + np.swapaxes(ZhT, -1, -2)


def _Z_from_exchange(eng, T):
    """Z[T] = K[T^T] ("ilkj,kl->ij")"""
    return eng.fock_jk(np.ascontiguousarray(np.swapaxes(np.asarray(T), -1, -2)))[1]


# ---- 2a: the geometry this file relies on ------------------------------------------------------------------------------------------------
def test_geometry_mirror_reaches_every_edge(engine):
    """If a formula of the library changes (block size, blocks per group, batch width, the slice size of (ab|ij)), this test fails instead
    of the others silently not reaching the edge any more."""
    engine.set_basis(_system("n2_ccpvtz")[1])
    N, csize, _ = _geometry(engine)
    g = _ladder_geometry(csize)
    print(f"\n[N2/cc-pVTZ] N {N} classes {csize} {g}")
    assert N == 60 and g["groups"] == 1 and g["passes"] == 1 and not g["second_block"], (csize, g)
    want = {200: {"nblk": 14, "groups": 1, "second_block": True, "passes": 3},
            400: {"nblk": 26, "groups": 2, "second_block": True, "passes": 6},
            520: {"groups": 3, "second_block": True}}
    for n in (200, 400, 520):
        engine.set_basis(_synthetic(n)[2])
        N, csize, _ = _geometry(engine)
        g = _ladder_geometry(csize)
        print(f"[synth-{n}] classes {csize} {g}")
        assert N == n and all(g[k] == x for k, x in want[n].items()), (n, csize, g)
        if n == 200:
            assert sorted(csize) == [22, 48, 48, 82]
            assert _abij_slices(200, 200 - 18) == [73, 73, 36]
        if n == 400:
            assert sorted(csize) == [46, 96, 96, 162] and g["last_rows"] == [2, 14, 16, 16]
            s18, s16 = _abij_slices(400, 400 - 18), _abij_slices(400, 400 - 16)     # (a frozen core keeps v, and so the slices)
            assert len(s18) == 48 and s18[-1] == 6 and set(s18[:-1]) == {8}
            assert s16 == [8] * 48


# ---- 2b: unit matrices -> tensor planes, exactly ----------------------------------------------------------------------------------------
def _unit_pairs(cls, n=TFL_W):
    """n pairs (la, si) of AOs (original indices) at the edges of the ladder kernel's loops: la == si; the first and last AO of each class;
    both sides of every 16-row block boundary (and so of every 32-column pass boundary) of the widest class; AOs of the last block of
    each class; la and si in the same and in different classes."""
    members = [np.flatnonzero(cls == c) for c in range(4)]
    wide = int(np.argmax([len(m) for m in members]))
    mw = members[wide]
    edges = sorted({0, len(mw) - 1} | {x for b in range(16, len(mw), 16) for x in (b - 1, b)})
    last_block = {c: [int(m[16 * ((len(m) - 1) // 16)]), int(m[-1])] for c, m in enumerate(members)}
    ends = [int(m[x]) for m in members for x in (0, -1)]
    pairs = [(a, a) for a in ends]                                    # la == si
    others = [a for c in range(4) for a in last_block[c]] + ends
    pairs += [(others[k % len(others)], int(mw[x])) for k, x in enumerate(edges)]          # si over the edges of the widest class
    pairs += [(int(mw[x]), others[(3 * k + 1) % len(others)]) for k, x in enumerate(edges[::2])]   # la over them
    for a in range(4):                                                # every ordered pair of classes, AOs of the last blocks
        for b in range(4):
            pairs.append((last_block[a][0], last_block[b][1]))
    rng = np.random.default_rng(64)
    out = []
    for p in pairs + [tuple(int(x) for x in rng.integers(0, len(cls), 2)) for _ in range(4 * n)]:
        if p not in out:
            out.append(p)
    return out[:n]


def test_unit_matrices_give_the_tensor_planes_exactly(engine):
    """synth-400: T_p = e_la e_si^T for 64 pairs (la, si) at the loop edges of the kernel -- one full batch -- and their transposes (a second
    batch).  Z_p[mu][nu] = (mu la|nu si) for ALL mu, nu against tf_sample_eri.  Every product in the kernel is value x 1 or value x 0, and
    the halved own pair comes back as 0.5 v + 0.5 v: the expected difference is zero (asserted <= 1e-15 max|plane|; whether it was bitwise
    is printed).  Where the four classes do not multiply to the identity the output must be an exact zero.  The message names the
    element."""
    t0 = time.perf_counter()
    engine.set_basis(_synthetic(400)[2]).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed"
    N = engine.N
    cls = _classes(engine)
    pairs = _unit_pairs(cls)
    assert len(pairs) == TFL_W == len(set(pairs))
    T = np.zeros((2 * TFL_W, N, N))
    for p, (la, si) in enumerate(pairs):
        T[p, la, si] = 1.0
        T[TFL_W + p, si, la] = 1.0
    Zh = engine.mp3_ladder_probe(T)
    Z = Zh[:TFL_W] + Zh[TFL_W:].transpose(0, 2, 1)
    kk, ll = _grid(N)
    bitwise, worst, bad = True, 0.0, []
    for p, (la, si) in enumerate(pairs):
        idx = np.stack([kk, np.full(N * N, la, np.int32), ll, np.full(N * N, si, np.int32)], axis=1)      # (mu la|nu si) at [mu][nu]
        plane = engine.sample_eri(idx).reshape(N, N)
        scale = float(np.abs(plane).max())
        d = np.abs(Z[p] - plane)
        if not np.array_equal(Z[p], plane):
            bitwise = False
        err = float(d.max()) if np.all(np.isfinite(d)) else float("inf")
        worst = max(worst, err / scale)
        forbidden = (cls[:, None] ^ cls[None, :] ^ cls[la] ^ cls[si]) != 0
        nz = np.argwhere(forbidden & (Z[p] != 0.0))
        if not err <= 1e-15 * scale:
            mu, nu = (int(x) for x in np.unravel_index(np.argmax(np.where(np.isfinite(d), d, np.inf)), d.shape))
            bad.append(f"p {p} (la {la}, si {si}; classes {cls[la]}, {cls[si]}): Z[{mu}][{nu}] = {Z[p, mu, nu]!r}, tensor {plane[mu, nu]!r}, "
                       f"err/max|plane| {err / scale:.2e}, {int(np.sum(~(d <= 1e-15 * scale)))} elements off")
        if len(nz):
            mu, nu = (int(x) for x in nz[0])
            bad.append(f"p {p} (la {la}, si {si}): Z[{mu}][{nu}] = {Z[p, mu, nu]!r} where the parity classes forbid a value ({len(nz)} such)")
    print(f"\n[synth-400 unit matrices] {len(pairs)} planes x {N * N} elements: worst err / max|plane| {worst:.2e}, bitwise {bitwise}, "
          f"{time.perf_counter() - t0:.1f} s")
    assert not bad, "\n".join(bad[:12])


# ---- 2c: random general matrices, the full output ---------------------------------------------------------------------------------------
def _random_matrices_case(eng, label):
    N = eng.N
    rng = np.random.default_rng(N)
    T = rng.standard_normal((TFL_W + 6, N, N))                     # one full batch and a batch of 6
    Z = _Z_from_probe(eng, T)
    Z1 = _Z_from_probe(eng, T[0])                                  # n = 1
    assert np.array_equal(eng.mp3_ladder_probe(T), eng.mp3_ladder_probe(T)), "the ladder kernel is not bitwise repeatable"
    K = _Z_from_exchange(eng, T)
    scale = np.abs(K).reshape(len(T), -1).max(axis=1)
    bad = []
    # (i) 24 elements against planes of the tensor, every matrix
    worst_i = 0.0
    for mu, nu in _picks(N, 17):
        M = _plane(eng, "akbl", mu, nu)                             # (mu k|nu l) at [k][l]
        ref = np.einsum("kl,pkl->p", M, T)
        for got, name in ((Z[:, mu, nu], "n = 70"), (Z1[None, mu, nu], "n = 1")):
            e = np.abs(got - ref[:len(got)]) / scale[:len(got)]
            worst_i = max(worst_i, float(np.nanmax(e)) if np.all(np.isfinite(e)) else float("inf"))
            for p in np.flatnonzero(~(e <= 1e-10)):
                bad.append(f"{label} {name}: Z_{p}[{mu}][{nu}] = {got[p]!r}, plane sum {ref[p]!r}, err/max|Z_p| {e[p]:.2e}")
    # (ii) every element against the exchange matrices
    d = np.abs(Z - K)
    e2 = d.reshape(len(T), -1).max(axis=1) / scale
    d1 = float(np.abs(Z1 - K[0]).max() / scale[0])
    worst_ii = max(float(e2.max()), d1) if np.all(np.isfinite(d)) and np.isfinite(d1) else float("inf")
    for p in np.flatnonzero(~(e2 <= 1e-10)):
        dp = np.where(np.isfinite(d[p]), d[p], np.inf)
        mu, nu = (int(x) for x in np.unravel_index(np.argmax(dp), dp.shape))
        bad.append(f"{label} n = 70: Z_{p}[{mu}][{nu}] = {Z[p, mu, nu]!r}, K[T^T] {K[p, mu, nu]!r}, err/max|Z_p| {e2[p]:.2e}, "
                   f"{int(np.sum(~(d[p] <= 1e-10 * scale[p])))} elements off")
    if not d1 <= 1e-10:
        bad.append(f"{label} n = 1: err/max|Z| {d1:.2e}")
    print(f"\n[{label} random matrices] worst err/max|Z_p|: 24 picks vs planes {worst_i:.2e}, all elements vs K[T^T] {worst_ii:.2e}")
    assert not bad, "\n".join(bad[:12])


def test_random_matrices_at_400_every_element(engine):
    """synth-400: 70 dense standard-normal non-symmetric matrices (a full batch and a batch of 6) and one matrix alone; (i) 24 elements of
    every Z_p against sum(plane * T_p), (ii) every element of every Z_p against the K of tf_fock_jk(T_p^T); 1e-10 max|Z_p|, the project's
    bound for J/K elements at this size; one call repeated must agree bitwise (one owner per output element, no atomics)."""
    engine.set_basis(_synthetic(400)[2]).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed" and engine.N == 400
    _random_matrices_case(engine, "synth-400")


def test_random_matrices_at_520_every_element():
    """the same at synth-520 (three block groups), in a context of its own"""
    with Engine(0) as eng:
        eng.set_basis(_synthetic(520)[2]).build_eri(True)
        assert eng.eri_storage()["layout"] == "packed" and eng.N == 520
        _random_matrices_case(eng, "synth-520")


# ---- 2d: the general-density exchange build -----------------------------------------------------------------------------------------------
def test_general_density_build_against_sampled_planes_and_across_layouts(engine):
    """tf_fock_jk of non-symmetric densities (two passes on the packed and tiles layouts), which the element-wise reference above and the
    rows / tiles routes of MP3 lean on: synth-400, packed and tiles, J and K of two densities -- one call each and both in one call -- at
    24 elements against planes of the tensor (1e-10 scale); synth-200, the rows layout against packed, every element (1e-11 scale, the
    bound of test_packed_and_rows_layouts_agree)."""
    rng = np.random.default_rng(2400)
    bad = []
    try:
        aos = _synthetic(400)[2]
        P = rng.standard_normal((2, 400, 400))
        planes = None
        for layout in ("packed", "tiles"):
            engine.set_basis(aos).build_eri(True, layout=layout)
            assert engine.eri_storage()["layout"] == layout and engine.N == 400
            if planes is None:
                planes = [(a, b, _plane(engine, "abkl", a, b), _plane(engine, "alkb", a, b)) for a, b in _picks(400, 17)]
            single = [engine.fock_jk(P[d]) for d in range(2)]
            J2, K2 = engine.fock_jk(P)
            worst = 0.0
            for d in range(2):
                for J, K, how in ((single[d][0], single[d][1], "alone"), (J2[d], K2[d], "both in one call")):
                    sJ, sK = float(np.abs(J).max()), float(np.abs(K).max())
                    for a, b, Mj, Mk in planes:
                        ej, ek = abs(J[a, b] - np.sum(Mj * P[d])) / sJ, abs(K[a, b] - np.sum(Mk * P[d])) / sK
                        worst = max(worst, ej, ek) if np.isfinite(ej) and np.isfinite(ek) else float("inf")
                        if not (ej <= 1e-10 and ek <= 1e-10):
                            bad.append(f"synth-400 {layout} density {d} ({how}): [{a}][{b}] J err {ej:.2e} K err {ek:.2e}")
            print(f"\n[synth-400 {layout} general densities] worst err/scale at 24 elements {worst:.2e}")
        aos = _synthetic(200)[2]
        P = rng.standard_normal((2, 200, 200))
        res = {}
        for layout in ("packed", "rows"):
            engine.set_basis(aos).build_eri(True, layout=layout)
            assert engine.eri_storage()["layout"] == layout and engine.N == 200
            res[layout] = [engine.fock_jk(P[0]), engine.fock_jk(P[1]), engine.fock_jk(P)]
        worst = 0.0
        for k in range(3):
            for q, name in enumerate("JK"):
                a, b = np.asarray(res["rows"][k][q]), np.asarray(res["packed"][k][q])
                e = float(np.abs(a - b).max() / np.abs(b).max())
                worst = max(worst, e) if np.isfinite(e) else float("inf")
                if not e <= 1e-11:
                    bad.append(f"synth-200 rows vs packed, call {k}, {name}: err/scale {e:.2e}")
        print(f"[synth-200 rows vs packed general densities] worst err/scale, every element {worst:.2e}")
    finally:
        _reset(engine)
    assert not bad, "\n".join(bad[:12])


# ---- 3: every MP3 term against NumPy --------------------------------------------------------------------------------------------------------
TERMS = ("E_pp", "E_hh", "E_ring")


def _reference_terms(eng, C, eps, o, frozen=(0,)):
    """{n_frozen: ((E_pp, E_hh, E_ring), (S_pp, S_hh, S_ring))} by mr.terms_from_blocks; no MP3 code of the library takes part: (ia|jb) from
    tf_ao_to_mo, (ij|ab) and (ki|lj) from symmetric Coulomb matrices, Z from general-density exchange matrices.  The frozen-core
    references are slices of the blocks of the full window."""
    Co, Cv = np.ascontiguousarray(C[:, :o]), np.ascontiguousarray(C[:, o:])
    ovov = eng.ao_to_mo(Co, Cv, Co, Cv)
    oovv, oooo = mr.blocks_from_coulomb(lambda D: eng.fock_jk(D)[0], Co, Cv)
    return {nf: mr.terms_from_blocks(np.ascontiguousarray(ovov[nf:, :, nf:, :]), oovv[nf:, nf:], oooo[nf:, nf:, nf:, nf:],
                                     lambda T: _Z_from_exchange(eng, T), Cv, eps[nf:o], eps[o:]) for nf in frozen}


def _check_terms(eng, C, eps, o, nf, ref, label, bad):
    """tf_mp3_rhf on the current layout: |got - ref| <= 1e-10 S per term, S = sum |t' X| of the reference (the bound the project uses
    between layouts at synth-400); E_OS, E_SS bit for bit those of tf_mp2_rhf"""
    r, m = eng.mp3_rhf(C, eps, o, nf), eng.mp2_rhf(C, eps, o, nf)
    E, S = ref
    for k, name in enumerate(TERMS):
        err = abs(r[name] - E[k])
        print(f"[{label}, {nf} frozen] {name} {r[name]:.12e} ref {E[k]:.12e} |d| {err:.2e} |d|/S {err / S[k]:.2e} (S {S[k]:.3e}) "
              f"|d|/|ref| {err / abs(E[k]):.2e}")
        if not err <= 1e-10 * S[k]:
            bad.append(f"{label}, {nf} frozen: {name} = {r[name]!r}, reference {E[k]!r}, |d|/S = {err / S[k]:.2e}")
    if not (r["E_OS"] == m["E_OS"] and r["E_SS"] == m["E_SS"]):
        bad.append(f"{label}, {nf} frozen: MP2 parts of tf_mp3_rhf {r['E_OS']!r}, {r['E_SS']!r} are not those of tf_mp2_rhf {m['E_OS']!r}, {m['E_SS']!r}")
    return r


def test_terms_at_400_bench_orbitals_and_frozen_core(engine, bench_orbitals):
    """synth-400, the converged orbitals of the bench leg, o = 18 ((ab|ij) in 48 slices, the last of 6; 324 pairs: five full batches and
    one of 4); 10 frozen (o = 8: exactly one full batch of 64 pairs) and 17 frozen (o = 1)."""
    t0 = time.perf_counter()
    aos, C, eps, o = bench_orbitals
    engine.set_basis(aos).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed" and engine.N == 400
    refs = _reference_terms(engine, C, eps, o, frozen=(0, 10, 17))
    t1 = time.perf_counter()
    bad, got = [], {}
    print()
    for nf in (0, 10, 17):
        got[nf] = _check_terms(engine, C, eps, o, nf, refs[nf], "synth-400 bench orbitals", bad)
    print(f"[synth-400 bench orbitals] reference {t1 - t0:.1f} s, library {time.perf_counter() - t1:.1f} s")
    assert not bad, "\n".join(bad)
    for nf in (10, 17):
        assert abs(got[nf]["E_MP3"] - got[0]["E_MP3"]) > 1e-6           # (the frozen orbitals did leave)


def test_terms_at_400_sixteen_occupied(engine):
    """synth-400, random orthonormal orbitals, o = 16: 256 pairs -- four full batches -- and (ab|ij) in 48 slices of exactly 8."""
    t0 = time.perf_counter()
    engine.set_basis(_synthetic(400)[2]).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed" and engine.N == 400
    C, eps = _random_orbitals(400, 416)
    refs = _reference_terms(engine, C, eps, 16)
    bad = []
    print()
    _check_terms(engine, C, eps, 16, 0, refs[0], "synth-400 random orbitals o = 16", bad)
    print(f"[synth-400 o = 16] {time.perf_counter() - t0:.1f} s")
    assert not bad, "\n".join(bad)


def test_terms_at_200_on_every_layout(engine):
    """synth-200, random orbitals, o = 18, on packed, tiles and rows: (ab|ij) in three slices (73, 73, 36), the ladder kernel with the second
    block of a wave and three column passes, and the exchange-build route of MP3 on the other two layouts."""
    aos = _synthetic(200)[2]
    C, eps = _random_orbitals(200, 218)
    bad = []
    try:
        engine.set_basis(aos).build_eri(True, layout="packed")
        refs = _reference_terms(engine, C, eps, 18)
        print()
        for layout in ("packed", "tiles", "rows"):
            engine.set_basis(aos).build_eri(True, layout=layout)
            assert engine.eri_storage()["layout"] == layout and engine.N == 200
            _check_terms(engine, C, eps, 18, 0, refs[0], f"synth-200 {layout}", bad)
    finally:
        _reset(engine)
    assert not bad, "\n".join(bad)
