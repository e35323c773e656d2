"""GPU: the three Fock-build kernel families -- jk_packed_kernel<1|2> with jk_reduce_kernel / jk_packed_final_kernel (tf_jkpacked.hip.h),
jk_tile_kernel<ND,MB,PF> with jk_edge_kernel / jk_tile_reduce_kernel (tf_jktile.hip.h) and jk_rows_kernel<NLC,JB,ND> -- on basis sets
whose parity-class widths sit on either side of the kernels' shape constants (tests/fock_reference.py: SHAPES), element by element:
  (a) the dense copy of the stored tensor against the CPU oracle (the writers xform_bra_store_packed / xform_bra_store_tiles);
  (b) unit densities P = E_kl + E_lk: J exactly E[:, :, k, l] + E[:, :, l, k] (= 2 E[:, :, k, l] on packed and tiles, whose copies are
      asserted symmetric bit for bit; the rows tensor is symmetric under k <-> l to an ulp only), K within three roundings of its two
      terms, parity zeros exact;
  (c) seeded random densities, symmetric and not, one to nine per call: |got - ref| <= (N*N + 4) 2^-53 A elementwise, A the absolute
      sum of the products (a bound for ANY order of the sum), the reference in np.longdouble (scf:55-72 "ijkl,kl->ij", scf:27-44
      "ilkj,kl->ij");
  (d) the same with the k walk cut in 2 and 3 parts (TF_JK_PARTS); (e) the device entry on a side stream;
the variants behind static environment reads in child processes; two ranks and a rank without rows on one card.
Bounds are derived (docstrings of fock_reference), the printed ratios are observations.  Every test hands the shared context back
with the default layout."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fock_reference as fr

pytestmark = pytest.mark.gpu

LAYOUTS = ("packed", "tiles", "rows")
TOL_INT = 1e-12
CASES = [(tag, True, lay) for tag in fr.SHAPES for lay in LAYOUTS] + [(tag, False, lay) for tag in fr.CARTESIAN_TAGS for lay in LAYOUTS]
NONSYM = 9                                                                 # index of the non-symmetric density in the pool
CALLS = [("1 sym", [0]), ("2 sym", [0, 1]), ("1 nonsym", [NONSYM]), ("sym+nonsym", [0, NONSYM]), ("sym+nonsym+sym", [0, NONSYM, 1])]
CALLS_TILES = [("4 sym", [0, 1, 2, 3]), ("5 sym", [0, 1, 2, 3, 4]), ("8 sym", list(range(8))), ("9 sym", list(range(9))),
               ("4 sym+nonsym", [0, 1, 2, 3, NONSYM])]
VARIANTS = [("packed", {"TF_JK_ONE_LAUNCH": "0"}), ("packed", {"TF_JK_ONE_LAUNCH": "0", "TF_JK_SERIAL": "1"}), ("packed", {"TF_JK_NOFUSE": "1"}),
            ("tiles", {"TF_TILE_KSUB": "64"}), ("tiles", {"TF_TILE_KSUB": "16"}), ("tiles", {"TF_TILE_PF": "1"})]
VARIANT_TAGS = ("two_s", "one_p", "c0_65", "mid_17_9")

# one shape at a time: the oracle tensor, the dense copies per layout and the longdouble references of the tensors seen so far
_CACHE = {"key": None}


def _cache(tag, sph):
    if _CACHE["key"] != (tag, sph):
        _CACHE.clear()
        _CACHE.update(key=(tag, sph), dense={}, refs=[])
    return _CACHE


def _reset(engine):
    engine._check(engine._L.tf_set_eri_layout(engine._ctx, -1))


def _oracle_tensor(tag, sph):
    c = _cache(tag, sph)
    if "oracle" not in c:
        from oracle import oracle as orc
        from ump2_reference import dense_eri
        _, shells, aos = fr.system(tag)
        c["oracle"] = dense_eri(aos, shells) if sph else orc.eri(aos)
    return c["oracle"]


def _pool(N):
    S, G = fr.random_densities(N, NONSYM)
    return np.concatenate([S, G[None]])


def _refs(tag, sph, E, n_pool=NONSYM + 1):
    """longdouble J, K and the absolute sums of the density pool for the dense tensor E: computed once per distinct tensor of a shape"""
    c = _cache(tag, sph)
    idx = list(range(n_pool - 1)) + [NONSYM]
    for E0, r in c["refs"]:
        if all(p in r["idx"] for p in idx) and np.array_equal(E0, E):
            return r
    pool = _pool(E.shape[0])
    out = fr.Reference(E).jk(pool[idx])
    r = {"pool": pool, "idx": {p: q for q, p in enumerate(idx)}, "J": out[0], "K": out[1], "AJ": out[2], "AK": out[3]}
    c["refs"].append((E, r))
    return r


def _build(engine, tag, sph, layout):
    _, shells, aos = fr.system(tag)
    engine.set_basis(aos).build_eri(sph, layout=layout)
    assert engine.eri_storage()["layout"] == layout
    L = fr.layout_of(shells, sph)
    assert engine.N == L.N
    return L


def _dense(engine, tag, sph, layout):
    """build the tensor in `layout` and return (class layout, dense copy); the copy is kept while the shape is the current one"""
    c = _cache(tag, sph)
    L = _build(engine, tag, sph, layout)
    if layout not in c["dense"]:
        c["dense"][layout] = engine.copy_eri()
    return L, c["dense"][layout]


def _first_bad(bad, names):
    n, i, j = (int(x) for x in np.argwhere(bad)[0])
    return f"{names[n]} output [{i},{j}] ({int(bad.sum())} elements in all)"


def run_unit_probes(fock, E, L, pairs, modes, where):
    """(b): every pair as a unit density, m per call for m in modes (exactly m: the list wraps around).  Returns the worst K ratio in
    units of 2^-53 S per mode; raises AssertionError naming layout, shape, output element and pair."""
    N, n = L.N, len(pairs)
    Jw, Kw, Sw = fr.unit_expectations(E, pairs)
    ks, ls = np.asarray([p[0] for p in pairs]), np.asarray([p[1] for p in pairs])
    forbidden = np.moveaxis(~fr.allowed_mask(L.cls)[:, :, ks, ls], 2, 0)
    assert np.all(Jw[forbidden] == 0.0) and np.all(Sw[forbidden] == 0.0)
    P = np.zeros((n, N, N))
    P[np.arange(n), ks, ls] = 1.0
    P[np.arange(n), ls, ks] = 1.0
    names = [f"pair (k, l) = ({k}, {l})" for k, l in pairs]
    worst = {}
    for m in modes:
        J, K = np.full((n, N, N), np.nan), np.full((n, N, N), np.nan)
        for s in range(0, n, m):
            idx = [(s + q) % n for q in range(m)]
            Jc, Kc = fock(P[idx[0]] if m == 1 else P[idx])
            J[idx], K[idx] = Jc, Kc
        tagm = f"{where}, {m} per call"
        bad = ~(J == Jw)
        assert not bad.any(), f"{tagm}: J is not exactly E[:, :, k, l] + E[:, :, l, k]: {_first_bad(bad, names)}"
        err = np.abs(K - Kw)
        bad = ~(err <= 4 * fr.EPS * Sw)
        assert not bad.any(), f"{tagm}: K beyond 4 x 2^-53 x S: {_first_bad(bad, names)}, worst {np.nanmax(err / np.where(Sw > 0, fr.EPS * Sw, np.nan)):.2f}"
        bad = forbidden & ~((J == 0.0) & (K == 0.0))
        assert not bad.any(), f"{tagm}: a parity-forbidden element is not 0.0: {_first_bad(bad, names)}"
        worst[m] = float(np.max(np.where(Sw > 0, err / np.where(Sw > 0, fr.EPS * Sw, 1.0), 0.0)))
    return worst


def run_random_calls(fock, N, refs, calls, where):
    """(c): the calls against the longdouble reference; then the first one-density call again, bit for bit.  Returns
    {call: (worst J ratio, worst K ratio)} in units of 2^-53 A; raises AssertionError naming the call and the element."""
    pool, bound = refs["pool"], fr.random_bound(N)
    out, first = {}, None
    for name, idx in calls:
        J, K = fock(pool[idx[0]] if len(idx) == 1 else pool[idx])
        J, K = J.reshape(len(idx), N, N), K.reshape(len(idx), N, N)
        if first is None:
            first = (idx, J.copy(), K.copy())
        q = [refs["idx"][p] for p in idx]
        ratios = []
        for what, got, ref, A in (("J", J, refs["J"][q], refs["AJ"][q]), ("K", K, refs["K"][q], refs["AK"][q])):
            err = np.abs(got - ref)
            bad = ~(err <= bound * A)
            names = [f"density {d} of the call" for d in range(len(idx))]
            worst = float(np.max(np.where(A > 0, err / np.where(A > 0, fr.EPS * A, 1.0), 0.0)))
            assert not bad.any(), f"{where}, call [{name}]: {what} beyond (N*N + 4) x 2^-53 x A = {N * N + 4}: {_first_bad(bad, names)}, worst ratio {worst:.1f}"
            ratios.append(worst)
        out[name] = tuple(ratios)
    idx, J0, K0 = first
    J, K = fock(pool[idx[0]])
    assert np.array_equal(J.reshape(J0.shape), J0) and np.array_equal(K.reshape(K0.shape), K0), f"{where}: the first call is not reproduced bit for bit after the others"
    return out


def _fmt(ratios):
    return ", ".join(f"{k}: J {a:.1f} K {b:.1f}" for k, (a, b) in ratios.items())


@pytest.mark.parametrize("tag,sph,layout", CASES, ids=[f"{t}-{'sph' if s else 'cart'}-{l}" for t, s, l in CASES])
def test_tensor_unit_probes_and_random_densities(engine, tag, sph, layout):
    where = f"layout {layout}, shape {tag} ({'spherical' if sph else 'Cartesian'})"
    try:
        if layout == "tiles" and "packed" not in _cache(tag, sph)["dense"]:
            _dense(engine, tag, sph, "packed")
        L, E = _dense(engine, tag, sph, layout)
        N = L.N
        # (a) the tensor
        Eo = _oracle_tensor(tag, sph)
        tol = TOL_INT * max(1.0, float(np.abs(Eo).max()))
        assert E.shape == Eo.shape and np.abs(E - Eo).max() <= tol, f"{where}: tensor off by {np.abs(E - Eo).max():.2e} (bound {tol:.1e})"
        assert np.all(E[~fr.allowed_mask(L.cls)] == 0.0), f"{where}: a parity-forbidden tensor element is not 0.0"
        if layout != "rows":                                                 # one stored image per element: J of a unit density is exactly 2 E[:, :, k, l]
            assert np.array_equal(E, E.transpose(0, 1, 3, 2)) and np.array_equal(E, E.transpose(1, 0, 2, 3)) and np.array_equal(E, E.transpose(2, 3, 0, 1))
        if layout == "tiles":
            assert np.array_equal(E, _cache(tag, sph)["dense"]["packed"]), f"{where}: the tiles copy differs from the packed one"
        # (b) unit densities
        pairs = fr.probe_pairs(L)
        unit = run_unit_probes(engine.fock_jk, E, L, pairs, (1, 2, 8) if layout == "tiles" else (1, 2), where)
        # (c) random densities
        rnd = run_random_calls(engine.fock_jk, N, _refs(tag, sph, E), CALLS + (CALLS_TILES if layout == "tiles" else []), where)
        print(f"\n[fock-shapes] {where}: N = {N}, {len(pairs)} unit probes, worst K ratio per densities-per-call {unit} (bound 4); "
              f"random densities (bound {N * N + 4}): {_fmt(rnd)}")
    finally:
        _reset(engine)


@pytest.mark.parametrize("parts", [2, 3])
@pytest.mark.parametrize("tag", ["c0_65", "mid_17_9"])
def test_cut_walks(engine, monkeypatch, tag, parts):
    """(d) TF_JK_PARTS (read at every build): the k walk of a packed task cut in 2 and 3 parts, the class of 65 and the classes of 17"""
    where = f"layout packed, TF_JK_PARTS={parts}, shape {tag}"
    monkeypatch.setenv("TF_JK_PARTS", str(parts))
    try:
        L = _build(engine, tag, True, "packed")
        E = engine.copy_eri()
        rnd = run_random_calls(engine.fock_jk, L.N, _refs(tag, True, E), CALLS, where)
        unit = run_unit_probes(engine.fock_jk, E, L, fr.probe_pairs(L), (1, 2), where)
        print(f"\n[fock-shapes] {where}: unit K {unit}; random densities (bound {L.N ** 2 + 4}): {_fmt(rnd)}")
    finally:
        monkeypatch.delenv("TF_JK_PARTS")
        _reset(engine)


PARENT_DROP_BYTES = 0      # free device memory after the third build minus after the sixth, measured on the commit before tf_jk_host.hip.h


def _free_device_memory():
    """hipMemGetInfo of the HIP runtime the library uses: the one mapped into this process -- the system's, or, where an earlier test
    imported torch first, the wheel's copy, which the library's dependency then resolved to.  With both mapped (torch imported after the
    library) the library's is the one outside the wheel."""
    import ctypes as C
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line}, key=lambda p: "/torch/" in p)
    assert paths, "no HIP runtime is mapped into this process"
    path = paths[0]
    free, total = C.c_size_t(), C.c_size_t()
    assert C.CDLL(path).hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_ownership_across_rebuilds(engine):
    """One context built packed -> tiles -> rows -> packed -> tiles -> rows on c0_65 (every block of the Fock state comes from one owner
    that free_eri clears; the cache recycles freed blocks at once, so a block freed twice would serve two later allocations).  After
    each build: fock_jk on the seeded symmetric pair and on the non-symmetric density; the second round's J and K equal the first
    round's bit for bit, per layout.  Free device memory after the sixth build is not lower than after the third by more than the
    commit before this test showed for the same sequence: PARENT_DROP_BYTES = 0 (measured on that commit's library with this test alone
    in the process and behind the c0_65 cases of this file: free memory 307 958 382 592 B and 307 895 468 032 B, each time the same
    after build 3 and after build 6)."""
    rounds, free = [], []
    try:
        for rnd in range(2):
            out = {}
            for layout in LAYOUTS:
                L = _build(engine, "c0_65", True, layout)
                pool = _pool(L.N)
                out[layout] = engine.fock_jk(pool[[0, 1]]) + engine.fock_jk(pool[NONSYM])
                assert all(np.isfinite(x).all() and np.abs(x).max() > 0 for x in out[layout]), (rnd, layout)
            rounds.append(out)
            free.append(_free_device_memory())
    finally:
        _reset(engine)
    print(f"\n[fock-shapes] rebuilds on c0_65: free device memory after build 3 {free[0]} B, after build 6 {free[1]} B, drop {free[0] - free[1]} B "
          f"(the parent's: {PARENT_DROP_BYTES} B)")
    for layout in LAYOUTS:
        for what, a, b in zip(("J sym pair", "K sym pair", "J nonsym", "K nonsym"), rounds[0][layout], rounds[1][layout]):
            assert np.array_equal(a, b), f"layout {layout}: {what} of the second round differs from the first"
    assert free[0] - free[1] <= PARENT_DROP_BYTES, (free, PARENT_DROP_BYTES)


def child_device_entry(layout):
    """What the child of test_device_entry_on_a_side_stream runs (torch initialises the device first, as in test_gpu_sharded.py: the
    wheel brings its own HIP runtime, which finds no device once the library's has the card)."""
    import torch
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    from tuna_amd.engine import Engine
    ok = {}
    with Engine(0) as eng:
        L = _build(eng, "mid_17_9", True, layout)
        pool = _pool(L.N)
        for nd in (1, 2):
            P = np.ascontiguousarray(pool[:nd])
            Jh, Kh = eng.fock_jk(P if nd > 1 else P[0])
            dP = torch.from_numpy(P).to("cuda:0")
            dJ, dK = torch.full_like(dP, float("nan")), torch.full_like(dP, float("nan"))
            torch.cuda.synchronize()
            eng.fock_jk_device(dP.data_ptr(), dJ.data_ptr(), dK.data_ptr(), nd, stream.cuda_stream)
            stream.synchronize()
            ok[str(nd)] = bool(np.array_equal(dJ.cpu().numpy().reshape(Jh.shape), Jh) and np.array_equal(dK.cpu().numpy().reshape(Kh.shape), Kh))
            ok[f"finite{nd}"] = bool(np.isfinite(Jh).all() and np.isfinite(Kh).all() and np.abs(Kh).max() > 0)
    print(json.dumps(ok))


def _child(call, env=None):
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_fock_shapes as t; t.%s" % (os.path.join(here, ".."), here, call)
    child_env = dict(os.environ)
    child_env.update(env or {})
    return subprocess.run([sys.executable, "-c", code], env=child_env, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("layout", ["packed", "tiles"])
def test_device_entry_on_a_side_stream(layout):
    """(e) tf_fock_jk_device with torch device tensors on a non-default stream: bit for bit tf_fock_jk, one and two symmetric densities
    on mid_17_9 (in a child process: see child_device_entry)"""
    out = _child("child_device_entry(%r)" % layout)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res == {"1": True, "finite1": True, "2": True, "finite2": True}, res


# ---- variants behind static environment reads: one fresh process each -------------------------------------------------------------

def child_main(layout):
    """What a child process runs: (b) on the edge pairs and (c) on VARIANT_TAGS in `layout`; prints one JSON line."""
    from tuna_amd.engine import Engine
    out = {}
    with Engine(0) as eng:
        for tag in VARIANT_TAGS:
            L = _build(eng, tag, True, layout)
            E = eng.copy_eri()
            where = f"layout {layout}, shape {tag}"
            aos = fr.edge_aos(L)
            pairs = [(k, l) for k in aos for l in aos if l <= k]
            try:
                unit = run_unit_probes(eng.fock_jk, E, L, pairs, (1, 2, 8) if layout == "tiles" else (1, 2), where)
                calls = CALLS + (CALLS_TILES if layout == "tiles" else [])
                rnd = run_random_calls(eng.fock_jk, L.N, _refs(tag, True, E, NONSYM + 1 if layout == "tiles" else 3), calls, where)
                out[tag] = {"N": L.N, "unit_K": max(unit.values()), "rand_J": max(a for a, _ in rnd.values()), "rand_K": max(b for _, b in rnd.values()),
                            "calls": {k: list(v) for k, v in rnd.items()}, "failure": None}
            except AssertionError as e:
                out[tag] = {"N": L.N, "failure": str(e)}
    print(json.dumps(out))


_CHILD_FAILED = []


@pytest.mark.parametrize("layout,env", VARIANTS, ids=[" ".join(f"{k}={v}" for k, v in e.items()) for _, e in VARIANTS])
def test_variants_behind_static_environment_reads(layout, env):
    """The three-launch bucketed path of the packed kernel (forked on side streams, and serial), the unfused two-density path, the
    64- and 16-row strips of the tiles kernel (jk_tile_kernel<1,4,1>, <1,1,*>) and its single-buffered loads (PF = 1): each in a fresh
    process, the children one after the other; the same bounds as above on what the child reports."""
    assert not _CHILD_FAILED, f"no further child is started after the failure of {_CHILD_FAILED[0]}"
    try:
        out = _child("child_main(%r)" % layout, env)
    except subprocess.TimeoutExpired:
        _CHILD_FAILED.append(env)
        raise
    if out.returncode != 0:
        _CHILD_FAILED.append(env)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert set(res) == set(VARIANT_TAGS)
    print(f"\n[fock-shapes] {env} ({layout}): " + "; ".join(f"{t}: unit K {r.get('unit_K')}, random J {r.get('rand_J')} K {r.get('rand_K')} (bound {r['N'] ** 2 + 4})"
                                                              for t, r in res.items()))
    for tag, r in res.items():
        assert r["failure"] is None, r["failure"]
        assert r["unit_K"] <= 4.0 and r["rand_J"] <= r["N"] ** 2 + 4 and r["rand_K"] <= r["N"] ** 2 + 4, (tag, r)


# ---- sharded tensors on one card --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["packed", "rows"])
@pytest.mark.parametrize("tag", ["c0_9", "c0_65", "mid_17_9"])
def test_two_ranks_on_one_card_add_up(tag, layout):
    """Engine(0, 0, 2) and Engine(0, 1, 2), one after the other in this process: the partial J and K of the two ranks added together
    satisfy the bound of (c) -- a split over ranks is only another order of the same sum.  The reference is contracted from the sum of
    the two ranks' dense copies (rows owned elsewhere read as zero)."""
    from tuna_amd.engine import Engine
    from tuna_amd import distributed as tdist
    _, shells, aos = fr.system(tag)
    owner = tdist.row_owner_matrix(shells, 2, layout=layout)
    partial, again, E, N = [], [], 0.0, 0
    for rank in (0, 1):
        with Engine(0, rank, 2) as eng:
            eng.set_basis(aos).build_eri(True, layout=layout)
            st = eng.eri_storage()
            assert st["layout"] == layout and st["rows"] == int((owner == rank).sum()) > 0
            N = eng.N
            pool = _pool(N)
            E = E + eng.copy_eri()
            partial.append([eng.fock_jk(pool[idx[0]] if len(idx) == 1 else pool[idx]) for _, idx in CALLS])
            again.append(eng.fock_jk(pool[CALLS[0][1][0]]))
            assert np.array_equal(again[-1][0], partial[-1][0][0]) and np.array_equal(again[-1][1], partial[-1][0][1])
    sums = iter([(a[0] + b[0], a[1] + b[1]) for a, b in zip(partial[0] + [again[0]], partial[1] + [again[1]])])
    where = f"two ranks, layout {layout}, shape {tag}"
    rnd = run_random_calls(lambda P: next(sums), N, _refs(tag, True, E, 3), CALLS, where)
    print(f"\n[fock-shapes] {where}: random densities (bound {N * N + 4}): {_fmt(rnd)}")


@pytest.mark.parametrize("layout", ["packed", "rows"])
def test_a_rank_without_rows(layout):
    """two_s on four ranks: three shell pairs, so one rank owns no row.  Its build succeeds, it stores nothing, and its partial J and K
    are all 0.0 (one and two densities, symmetric and not)."""
    from tuna_amd.engine import Engine
    from tuna_amd import distributed as tdist
    _, shells, aos = fr.system("two_s")
    owner = tdist.row_owner_matrix(shells, 4, layout=layout)
    idle = [r for r in range(4) if not (owner == r).any()]
    assert idle, owner
    pool = _pool(2)
    with Engine(0, idle[0], 4) as eng:
        eng.set_basis(aos).build_eri(True, layout=layout)
        assert eng.eri_storage()["rows"] == 0 and eng.eri_storage()["layout"] == layout
        assert np.all(eng.copy_eri() == 0.0)
        for name, idx in CALLS:
            J, K = eng.fock_jk(pool[idx[0]] if len(idx) == 1 else pool[idx])
            assert np.all(J == 0.0) and np.all(K == 0.0), (layout, name, J, K)
