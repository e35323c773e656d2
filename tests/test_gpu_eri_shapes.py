"""GPU: the launch structure of tf_build_eri (EriBuild in tf_eri_host.hip.h) -- forced slab cuts, every ERI kernel family, the seams of
the Boys function -- element by element against the CPU oracle.  The systems, slab settings and seam geometries are in
tests/eri_shapes.py; Engine.eri_build_stats() (tf_eri_build_stats) tells which path a build took.
  (a) slab cuts: one slab, TF_SLAB_MB=1, TF_SLAB_ROWS=R_mid and TF_SLAB_ROWS=1 (one bra shell pair per slab) in both ERI modes on the
      three layouts: the dense tensor against the oracle, parity zeros exact, and against the one-slab build of the same mode and layout;
  (b) families of generally contracted shell pairs under cuts;  (c) the buffers a context keeps from build to build;
  (d) two ranks on one card;  (e) the variants behind static environment reads, one child process each;
  (f) the seam system at every distance of eri_shapes.seam_distances(): whole tensors and the one-electron matrices.
Bounds: TOL_INT = 1e-12 absolute on O(1) integrals (scaled by max(1, max |oracle|)), 1e-10 on J and K, as tests/test_gpu_parity.py.
DESIGN.md section 4.2c lists what each case reaches and the deviations measured."""
import json
import os
import subprocess
import sys
from contextlib import contextmanager

import numpy as np
import pytest

import eri_shapes as es
from conftest import atom_arrays

pytestmark = pytest.mark.gpu

TOL_INT = 1e-12
TOL_JK = 1e-10
MODES = ("generic", "class")
LAYOUTS = ("packed", "tiles", "rows")
TEAM_KEYS = ("team16", "team64", "team256")
CFACT_KEYS = ("cfact_uncontracted", "cfact_contracted", "cfact_gtab", "cfact_ket_families", "cfact_both_families", "cfact_bra_families")
ROUND2_KEYS = ("multi", "fact", "class_staged", "class_unstaged")
SLAB_CASES = [(tag, True, lay) for tag in es.SLAB_TAGS for lay in LAYOUTS] + \
             [(tag, False, lay) for tag in es.CARTESIAN_SLAB_TAGS for lay in ("packed", "rows")]
FAMILY_ENVS = [{"TF_ERI_FAMILIES": "1"}, {"TF_ERI_FAMILIES": "1", "TF_ERI_CC_FAMILIES": "0"},
               {"TF_ERI_FAMILIES": "1", "TF_ERI_BRA_FAMILIES": "1"}, {"TF_ERI_FAMILIES": "0"}]


@contextmanager
def _env(env):
    """environment variables that tf_build_eri reads at every build"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _reset(engine):
    engine._check(engine._L.tf_set_eri_layout(engine._ctx, -1))


def _tol(Eo):
    return TOL_INT * max(1.0, float(np.abs(Eo).max()))


def _first(bad):
    return tuple(int(x) for x in np.argwhere(bad)[0])


def build_checked(eng, tag, sph, layout, env, where, forbidden=None):
    """One build under `env`: (dense copy, stats, worst |GPU - oracle|); asserts the tensor against the oracle and the parity zeros"""
    _, shells, aos = es.system(tag)
    with _env(env):
        eng.set_basis(aos).build_eri(sph, layout=layout)
    st = eng.eri_build_stats()
    assert eng.eri_storage()["layout"] == layout
    E, Eo = eng.copy_eri(), es.oracle_tensor(tag, sph)
    assert E.shape == Eo.shape
    err = np.abs(E - Eo)
    dev = float(np.nanmax(err)) if np.isfinite(err).all() else float("inf")
    bad = ~(err <= _tol(Eo))
    assert not bad.any(), f"{where}: element {_first(bad)} is {E[_first(bad)]!r}, oracle {Eo[_first(bad)]!r}; {int(bad.sum())} elements beyond {_tol(Eo):.1e}, worst {dev:.3e}"
    if forbidden is None:
        forbidden = es.parity_forbidden(shells, sph)
    bad = forbidden & (E != 0.0)
    assert not bad.any(), f"{where}: parity-forbidden element {_first(bad)} is {E[_first(bad)]!r}, not 0.0"
    launches = sum(st[k] for k in TEAM_KEYS + ("teamc",) + CFACT_KEYS + ("component_lane",) + ROUND2_KEYS)
    assert st["launches"] == launches > 0 and st["team_flat"] <= sum(st[k] for k in TEAM_KEYS), st
    return E, st, dev


def check_mode_families(st, mode, layout, uncontracted, where):
    """which kernel families a mode may launch by default"""
    if mode == "generic":
        assert sum(st[k] for k in TEAM_KEYS + ROUND2_KEYS + ("teamc",)) == 0 and sum(st[k] for k in CFACT_KEYS + ("component_lane",)) > 0, (where, st)
    else:
        assert sum(st[k] for k in CFACT_KEYS + ("component_lane", "teamc")) == 0, (where, st)
        if layout == "rows":
            assert sum(st[k] for k in TEAM_KEYS) == 0 and sum(st[k] for k in ROUND2_KEYS) > 0, (where, st)
        elif uncontracted:
            assert sum(st[k] for k in TEAM_KEYS) == st["launches"], (where, st)


def check_jk(eng, tag, sph, where):
    from oracle import scf_oracle as so
    Eo = es.oracle_tensor(tag, sph)
    rng = np.random.default_rng(5)
    A = rng.standard_normal((eng.N, eng.N))
    P = A + A.T
    J, K = eng.fock_jk(P)
    dj, dk = float(np.abs(J - so.coulomb(P, Eo)).max()), float(np.abs(K - so.exchange(P, Eo)).max())
    assert dj <= TOL_JK and dk <= TOL_JK, f"{where}: J off by {dj:.2e}, K by {dk:.2e}"
    return dj, dk


# ---- (a) slab cuts ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,sph,layout", SLAB_CASES, ids=[f"{t}-{'sph' if s else 'cart'}-{l}" for t, s, l in SLAB_CASES])
def test_slab_cuts(engine, tag, sph, layout):
    """The slab loop of run_slab: the cut of the class-sorted bra list into runs, the two sets of index lists, d_C and d_T2 reused from slab
    to slab, bra families and task lists rebuilt per slab, class runs split by a cut.  f_mix (one primitive quartet per element, nothing
    a cut changes enters its arithmetic) must come out bit for bit as in one slab; the contracted systems within TOL_INT of it (q.npq of
    a run sizes the primitive batches of eri_class_kernel, the families of a slab group other pairs), the difference printed."""
    _, shells, _ = es.system(tag)
    forbidden = es.parity_forbidden(shells, sph)
    uncontracted = all(len(s.exps) == 1 for s in shells)
    lines = []
    try:
        for mode in MODES:
            one = None
            for name, env, slabs_ok in es.slab_settings(shells):
                where = f"{tag} ({'spherical' if sph else 'Cartesian'}), TF_ERI_MODE={mode}, layout {layout}, {name}"
                E, st, dev = build_checked(engine, tag, sph, layout, dict(env, TF_ERI_MODE=mode), where, forbidden)
                assert slabs_ok(st["slabs"]), f"{where}: {st['slabs']} slabs"
                check_mode_families(st, mode, layout, uncontracted, where)
                if one is None:
                    one, diff = E, 0.0
                else:
                    diff = float(np.abs(E - one).max())
                    if tag == "f_mix":
                        bad = E != one
                        assert not bad.any(), f"{where}: element {_first(bad)} differs from the one-slab build by {diff:.3e} ({int(bad.sum())} elements)"
                    else:
                        assert diff <= _tol(one), f"{where}: differs from the one-slab build by {diff:.3e}"
                lines.append(f"{mode:7s} {name:20s} slabs {st['slabs']:3d} launches {st['launches']:5d} |GPU - oracle| {dev:.2e} |cut - one slab| {diff:.2e}")
                if name == "TF_SLAB_ROWS=1" and mode == MODES[-1]:
                    dj, dk = check_jk(engine, tag, sph, where)
                    lines.append(f"        fock_jk after it: J {dj:.2e} K {dk:.2e}")
        print(f"\n[eri-shapes] (a) {tag} {'sph' if sph else 'cart'} {layout}:\n  " + "\n  ".join(lines))
    finally:
        _reset(engine)


@pytest.mark.parametrize("tag", es.TINY_TAGS)
def test_tiny_shapes_one_pair_per_slab(engine, tag):
    """N = 1, 2, 3, 5 with TF_SLAB_ROWS=1 in both modes on the three layouts"""
    _, shells, _ = es.system(tag)
    try:
        for mode in MODES:
            for layout in LAYOUTS:
                where = f"{tag}, TF_ERI_MODE={mode}, layout {layout}, TF_SLAB_ROWS=1"
                _, st, _ = build_checked(engine, tag, True, layout, {"TF_ERI_MODE": mode, "TF_SLAB_ROWS": "1"}, where)
                assert st["slabs"] == es.n_bra_pairs(shells), (where, st)
    finally:
        _reset(engine)


def test_deep_contraction_in_both_modes(engine):
    """deep_p, one p shell of ten primitives: in per-class mode the Hermite tables of (pp|pp) do not fit what eri_class_kernel stages
    in LDS (eri_class_kernel<false, false>, the tables read from global memory)"""
    try:
        for mode in MODES:
            for layout in ("packed", "rows"):
                for sph in (True, False):
                    where = f"deep_p ({'spherical' if sph else 'Cartesian'}), TF_ERI_MODE={mode}, layout {layout}"
                    _, st, dev = build_checked(engine, "deep_p", sph, layout, {"TF_ERI_MODE": mode}, where)
                    assert (st["class_unstaged"] > 0 and st["class_staged"] == 0) if mode == "class" else st["cfact_contracted"] > 0, (where, st)
                    print(f"\n[eri-shapes] {where}: |GPU - oracle| {dev:.2e}, {st}")
    finally:
        _reset(engine)


# ---- (b) families x cuts --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("env", FAMILY_ENVS, ids=[" ".join(f"{k}={v}" for k, v in e.items()) for e in FAMILY_ENVS])
def test_families_under_slab_cuts(engine, env):
    """c2_n2_ccpvtz with the environments of test_families_of_generally_contracted_shell_pairs, cut at R_mid and into single bra pairs:
    bra_families() is rebuilt per (slab, bra group), the ket families are the build's"""
    tag = "c2_n2_ccpvtz"
    _, shells, _ = es.system(tag)
    forbidden = es.parity_forbidden(shells, True)
    want = {"cfact_ket_families": env["TF_ERI_FAMILIES"] == "1", "cfact_both_families": env["TF_ERI_FAMILIES"] == "1" and "TF_ERI_CC_FAMILIES" not in env,
            "cfact_bra_families": "TF_ERI_BRA_FAMILIES" in env}
    try:
        for name, cut, slabs_ok in es.slab_settings(shells)[2:]:
            where = f"{tag}, {env}, {name}"
            _, st, dev = build_checked(engine, tag, True, "packed", dict(env, **cut), where, forbidden)
            assert slabs_ok(st["slabs"]), (where, st)
            for key, on in want.items():
                assert (st[key] > 0) == on, (where, key, st)
            assert st["cfact_contracted"] > 0 or env["TF_ERI_FAMILIES"] == "1", (where, st)
            print(f"\n[eri-shapes] (b) {where}: slabs {st['slabs']}, |GPU - oracle| {dev:.2e}, " + ", ".join(f"{k} {st[k]}" for k in CFACT_KEYS))
    finally:
        _reset(engine)


# ---- (c) buffer reuse across builds of one context ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_buffers_kept_from_build_to_build(engine, mode):
    """The scratch slabs, the tensor buffer and the streams and events of a context outlive a build: a large tensor cut into single pairs,
    a small one in one slab, the large one again at R_mid and once more in single pairs -- the last build equals the first bit for bit"""
    hl = es.system("high_l")[1]
    seq = [("high_l", {"TF_SLAB_ROWS": "1"}, es.n_bra_pairs(hl)), ("n2_ccpvdz", {}, 1), ("high_l", {"TF_SLAB_ROWS": str(es.r_mid(hl))}, None),
           ("high_l", {"TF_SLAB_ROWS": "1"}, es.n_bra_pairs(hl))]
    try:
        kept = []
        for tag, cut, slabs in seq:
            where = f"TF_ERI_MODE={mode}, {tag}, {cut or 'one slab'}"
            E, st, dev = build_checked(engine, tag, True, "packed", dict(cut, TF_ERI_MODE=mode), where)
            assert st["slabs"] == slabs if slabs is not None else st["slabs"] >= 3, (where, st)
            kept.append(E)
            print(f"\n[eri-shapes] (c) {where}: slabs {st['slabs']}, |GPU - oracle| {dev:.2e}")
        assert np.array_equal(kept[0], kept[3]), f"TF_ERI_MODE={mode}: the last build differs from the first by {np.abs(kept[0] - kept[3]).max():.3e}"
    finally:
        _reset(engine)


@pytest.mark.parametrize("env", [{"TF_ERI_NSTREAM": "1", "TF_ERI_MODE": "generic"}, {"TF_ERI_NSTREAM": "1", "TF_ERI_MODE": "class"},
                                 {"TF_ERI_NQ": "1", "TF_ERI_MODE": "generic"}], ids=["NSTREAM=1 generic", "NSTREAM=1 class", "NQ=1 generic"])
def test_one_stream_and_one_queue(engine, env):
    """TF_ERI_NSTREAM=1 and TF_ERI_NQ=1 (read per build): every launch of a slab on one stream, c2_n2_ccpvtz cut at R_mid"""
    shells = es.system("c2_n2_ccpvtz")[1]
    try:
        where = f"c2_n2_ccpvtz, {env}, TF_SLAB_ROWS=R_mid"
        _, st, dev = build_checked(engine, "c2_n2_ccpvtz", True, "packed", dict(env, TF_SLAB_ROWS=str(es.r_mid(shells))), where)
        assert st["slabs"] >= 3, st
        print(f"\n[eri-shapes] (c) {where}: slabs {st['slabs']}, |GPU - oracle| {dev:.2e}")
    finally:
        _reset(engine)


# ---- (d) two ranks on one card ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag", ["c2_n2_ccpvtz", "f_mix"])
def test_two_ranks_cut_at_r_mid(tag, mode):
    """Engine(0, 0, 2) and Engine(0, 1, 2), one after the other: each rank cuts its own bra pairs (mine_sorted) at R_mid; the sum of the
    two dense copies is the tensor (rows owned elsewhere read as zero)"""
    from tuna_amd.engine import Engine
    _, shells, aos = es.system(tag)
    R = es.r_mid(shells)
    Eo = es.oracle_tensor(tag, True)
    E, lines = 0.0, []
    for rank in (0, 1):
        rows, pairs = es.rank_rows(shells, rank, 2), es.n_bra_pairs(shells, rank, 2)
        with Engine(0, rank, 2) as eng, _env({"TF_ERI_MODE": mode, "TF_SLAB_ROWS": str(R)}):
            eng.set_basis(aos).build_eri(True, layout="packed")
            st = eng.eri_build_stats()
            E = E + eng.copy_eri()
        # a slab takes pairs until the next one would pass R: two consecutive slabs hold more than R rows
        assert -(-rows // R) <= st["slabs"] <= min(pairs, 2 * -(-rows // R) + 1) and st["slabs"] >= 2, (tag, mode, rank, rows, R, st)
        lines.append(f"rank {rank}: {pairs} pairs, {rows} rows, {st['slabs']} slabs")
    dev = float(np.abs(E - Eo).max())
    print(f"\n[eri-shapes] (d) {tag}, TF_ERI_MODE={mode}, TF_SLAB_ROWS={R}: " + "; ".join(lines) + f"; |sum of the ranks - oracle| {dev:.2e}")
    assert dev <= _tol(Eo), (tag, mode, dev)
    assert np.all(E[es.parity_forbidden(shells, True)] == 0.0)


# ---- (e) variants behind static environment reads: one fresh process each ---------------------------------------------------------------

CHILD_TAGS = ("f_mix", "n2_ccpvdz", "high_l", "one_d", es.seam_tag(6.0))
SEAM_EXTRA = tuple(es.seam_tag(R) for R in (float(np.nextafter(6.0, 0.0)), float(np.nextafter(6.0, 7.0)), 12.0))
TEAMC = {"TF_ERI_TEAMC": "1"}
# (mode, environment, also the seam geometries around T = 36)
VARIANTS = [("generic", TEAMC, True), ("generic", dict(TEAMC, TF_TEAMC_PQMAX="1"), True), ("generic", dict(TEAMC, TF_TEAMC_PQMAX="100000"), True),
            ("class", {"TF_ERI_TEAM": "0"}, True), ("class", {"TF_ERI_TEAM": "0", "TF_ERI_NOFACT": "1"}, True),
            ("class", {"TF_ERI_TEAM_SIZE": "16"}, False), ("class", {"TF_ERI_TEAM_SIZE": "64"}, False), ("class", {"TF_ERI_TEAM_SIZE": "256"}, False),
            ("class", {"TF_TEAM_KPW_DIV": "1"}, False), ("class", {"TF_TEAM_KPW_MAX": "1"}, False),
            ("class", {"TF_TEAM_LDS_KB": "8", "TF_TEAM16_NNZ": "0"}, False), ("generic", {"TF_ERI_GENERIC_OLD": "1"}, False)]


def child_main(mode, extra_seams):
    """What a child process runs: CHILD_TAGS spherical and Cartesian, in one slab and at R_mid, in `mode` on the packed layout (and the
    seam geometries around T = 36 in one slab); prints one JSON line {case: {"dev", "tol", "stats", "failure"}}."""
    from tuna_amd.engine import Engine
    out = {}
    with Engine(0) as eng:
        for tag in CHILD_TAGS + (SEAM_EXTRA if extra_seams else ()):
            _, shells, _ = es.system(tag)
            cuts = [("one slab", {})] + ([("R_mid", {"TF_SLAB_ROWS": str(es.r_mid(shells))})] if tag in CHILD_TAGS else [])
            for sph in (True, False):
                forbidden = es.parity_forbidden(shells, sph)
                for name, cut in cuts:
                    case = f"{tag} {'sph' if sph else 'cart'} {name}"
                    try:
                        _, st, dev = build_checked(eng, tag, sph, "packed", dict(cut, TF_ERI_MODE=mode), case, forbidden)
                        out[case] = {"dev": dev, "tol": _tol(es.oracle_tensor(tag, sph)), "stats": st, "failure": None}
                    except AssertionError as e:
                        out[case] = {"dev": None, "stats": eng.eri_build_stats(), "failure": str(e)[:600]}
            es.drop_oracle(tag)
    print(json.dumps(out))


def _child(call, env=None):
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_eri_shapes as t; t.%s" % (os.path.join(here, ".."), here, call)
    child_env = dict(os.environ)
    child_env.update(env or {})
    return subprocess.run([sys.executable, "-c", code], env=child_env, capture_output=True, text=True, timeout=600)


_CHILD_FAILED = []


def _sum(st, keys):
    return sum(st[k] for k in keys)


def check_variant(env, res):
    """what the stats of a variant's builds must show (res: the child's report)"""
    fmix = {c: r["stats"] for c, r in res.items() if c.startswith("f_mix")}
    every = {c: r["stats"] for c, r in res.items()}
    if "TF_ERI_TEAMC" in env:
        for c, st in every.items():
            assert st["teamc"] > 0 and _sum(st, TEAM_KEYS + ROUND2_KEYS) == 0, (c, st)
        for c, st in fmix.items():                                          # uncontracted, every pair sum <= TF_TEAM_LMAX: nothing is left for eri_cfact_kernel
            assert st["launches"] == st["teamc"], (c, st)
    elif env.get("TF_ERI_TEAM") == "0":
        tot = {k: sum(st[k] for st in every.values()) for k in TEAM_KEYS + ROUND2_KEYS}
        assert _sum(tot, TEAM_KEYS) == 0 and tot["multi"] > 0 and tot["class_staged"] > 0, tot
        assert (tot["fact"] == 0) if "TF_ERI_NOFACT" in env else (tot["fact"] > 0), tot
        for c, st in every.items():
            assert _sum(st, ROUND2_KEYS) == st["launches"], (c, st)
    elif "TF_ERI_TEAM_SIZE" in env:
        size = int(env["TF_ERI_TEAM_SIZE"])
        launched = es.team_class_launches(es.system("f_mix")[1])
        want = sum(es.team_size_instantiated(lab, lcd, size) for lab, lcd in launched)
        for c, st in fmix.items():
            assert _sum(st, TEAM_KEYS) == st["launches"], (c, st)
            if c.endswith("one slab"):
                assert st["launches"] == len(launched) and st[f"team{size}"] == want > 0, (c, size, want, len(launched), st)
            else:
                assert st[f"team{size}"] > 0, (c, st)
    elif "TF_TEAM_LDS_KB" in env:
        for c, st in fmix.items():
            assert st["team256"] > 0 and st["team16"] == 0 and st["team_flat"] < _sum(st, TEAM_KEYS), (c, st)
    elif "TF_ERI_GENERIC_OLD" in env:
        for c, st in every.items():
            assert st["component_lane"] == st["launches"], (c, st)
    else:                                                                   # TF_TEAM_KPW_*: the same launches, another walk inside them
        for c, st in fmix.items():
            assert _sum(st, TEAM_KEYS) == st["launches"], (c, st)


@pytest.mark.parametrize("mode,env,seams", VARIANTS, ids=[" ".join(f"{k}={v}" for k, v in e.items()) for _, e, _ in VARIANTS])
def test_variants_behind_static_environment_reads(mode, env, seams):
    """eri_teamc_kernel over task lists (with the quartets split between it and eri_cfact_kernel at 700, 1 and 100000 primitive quartets),
    the round-2 per-class kernels eri_multi_kernel / eri_fact_kernel / eri_class_kernel with the team kernels off, the three team sizes
    forced, workgroups that walk many ket groups and exactly one, the blocked (non-flat) component lists under a small LDS limit, and the
    component-per-lane kernel: each in a fresh process, the children one after the other; no further child once one has ended abnormally."""
    assert not _CHILD_FAILED, f"no further child is started after the failure of {_CHILD_FAILED[0]}"
    try:
        out = _child("child_main(%r, %r)" % (mode, seams), env)
    except subprocess.TimeoutExpired:
        _CHILD_FAILED.append(env)
        raise
    if out.returncode != 0:
        _CHILD_FAILED.append(env)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert len(res) == 4 * len(CHILD_TAGS) + (2 * len(SEAM_EXTRA) if seams else 0)
    fam = {k: sum(r["stats"][k] for r in res.values()) for k in next(iter(res.values()))["stats"] if k != "slabs"}
    print(f"\n[eri-shapes] (e) {env} ({mode}): worst |GPU - oracle| / bound {max((r['dev'] or 0.0) / r.get('tol', 1.0) for r in res.values()):.3f}; launches "
          + ", ".join(f"{k} {v}" for k, v in fam.items() if v)
          + "".join(f"\n  {c}: {r['dev']} " + ", ".join(f"{k} {v}" for k, v in r["stats"].items() if v) for c, r in res.items()))
    for case, r in res.items():
        assert r["failure"] is None, r["failure"]
        assert r["dev"] <= r["tol"], (case, r)
        if case.endswith("R_mid"):
            assert r["stats"]["slabs"] >= (3 if not case.startswith("one_d") else 1), (case, r["stats"])
    check_variant(env, res)


# ---- (f) Boys seams and geometries -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", es.seam_distances(), ids=[f"R={R!r}" for R in es.seam_distances()])
def test_seam_geometries(engine, R):
    """The seam system at distance R in both modes on the packed layout: whole Cartesian and spherical tensors and the Cartesian
    one-electron matrices against the oracle; at R = 200 every element with a pair that straddles the centres is exactly the oracle's 0.0
    and the tensor is finite.  T of its probe quartets sits at 0 with R != 0, on either side of the rounding of the Boys
    grid index, in the last grid row and at the first value of the asymptotic branch (tests/test_eri_shapes.py asserts that of the list)."""
    from oracle import oracle as orc
    tag = es.seam_tag(R)
    atoms, shells, aos = es.system(tag)
    lines = []
    try:
        for sph in (False, True):
            forbidden = es.parity_forbidden(shells, sph)
            for mode in MODES:
                where = f"seam system at R = {R!r} ({'spherical' if sph else 'Cartesian'}), TF_ERI_MODE={mode}"
                E, st, dev = build_checked(engine, tag, sph, "packed", {"TF_ERI_MODE": mode}, where, forbidden)
                lines.append(f"{'sph' if sph else 'cart'} {mode}: {dev:.2e}")
                if R == 200.0:
                    Eo = es.oracle_tensor(tag, sph)
                    centre = np.asarray([s.atom for s in shells for _ in range(s.n_sph if sph else s.n_cart)])
                    straddles = centre[:, None] != centre[None, :]                  # a pair with one function on each centre: its overlap underflows
                    between = straddles[:, :, None, None] | straddles[None, None, :, :]
                    assert np.isfinite(E).all(), where
                    bad = between & (Eo == 0.0) & (E != 0.0)
                    assert not bad.any(), f"{where}: element {_first(bad)} is {E[_first(bad)]!r} where the oracle gives 0.0 ({int(bad.sum())} elements)"
                del E
        xyz, chg, org = atom_arrays(atoms)
        engine.set_basis(aos)
        ref = orc.one_electron(aos, xyz, chg, org, threads=min(16, os.cpu_count() or 1))
        for got, want, name in zip(engine.one_electron(xyz, chg, org, spherical=False), ref, "STVDQ"):
            d = float(np.abs(got - want).max()) if np.isfinite(got).all() else float("inf")
            assert d <= TOL_INT * max(1.0, float(np.abs(want).max())), f"seam system at R = {R!r}: {name} off by {d:.3e}"
            lines.append(f"{name} {d:.1e}")
        print(f"\n[eri-shapes] (f) R = {R!r}, T = {es.probe_T(R)}: |GPU - oracle| " + ", ".join(lines))
    finally:
        es.drop_oracle(tag)
        _reset(engine)


# ---- (g) the lifetimes of a context: created and destroyed many times, a refused basis between two good ones ---------------------------------

def test_context_rounds_and_refused_basis():
    """Twenty contexts in one process, each created, given a basis, built and closed (H2/STO-3G and a four-shell s,p basis in turn, the
    three layouts in turn): every tensor equals the first of its kind bit for bit.  Then one context: a basis and a build; tf_set_basis
    refused for a centre off the z axis and for a null argument, after each of which tf_one_electron, tf_build_eri and tf_dims refuse with
    their codes and texts; the first basis again, whose tensor and S, T, V equal those of a fresh context bit for bit."""
    import ctypes
    from conftest import R_H2
    from tuna_amd import molecule as mol
    from tuna_amd._lib import TunaError, ptr
    from tuna_amd.engine import Engine
    atoms = mol.make_atoms(["H", "H"], R_H2)
    bases = [mol.expand_cartesian_aos(mol.build_shells(atoms, "STO-3G")),
             mol.expand_cartesian_aos(mol.build_shells(atoms, {1: [("S", [(1.2, 1.0)]), ("P", [(0.8, 1.0)])]}))]
    xyz, chg, org = atom_arrays(atoms)
    first = {}
    for rnd in range(20):
        b, layout = rnd % 2, LAYOUTS[rnd % 3]
        with Engine(0) as eng:
            E = eng.set_basis(bases[b]).build_eri(True, layout).copy_eri()
        assert E.shape == ((2,) * 4 if b == 0 else (8,) * 4) and np.isfinite(E).all() and np.abs(E).max() > 0.1
        assert np.array_equal(E, first.setdefault((b, layout), E)), f"round {rnd}: basis {b}, layout {layout} differs from its first build"
    assert len(first) == 6

    EINVAL, EGEOM = -1, -6
    with Engine(0) as fresh:
        E_ref = fresh.set_basis(bases[1]).build_eri(True, "packed").copy_eri()
        STV_ref = fresh.one_electron(xyz, chg, org)[:3]
    with Engine(0) as eng:
        L, ctx = eng._L, eng._ctx
        last = lambda: L.tf_last_error(ctx).decode()
        assert np.array_equal(eng.set_basis(bases[1]).build_eri(True, "packed").copy_eri(), E_ref)
        good = eng._keep

        def refused_everywhere():
            S, T, V = np.zeros((8, 8)), np.zeros((8, 8)), np.zeros((8, 8))
            x, c, o = (np.ascontiguousarray(v, dtype=np.float64) for v in (np.asarray(xyz).reshape(-1, 3), chg, org))
            assert L.tf_one_electron(ctx, 2, ptr(x), ptr(c), ptr(o), 1, ptr(S), ptr(T), ptr(V), None, None) == EINVAL
            assert last() == "tf_one_electron: call tf_set_basis first"
            assert L.tf_build_eri(ctx, 1) == EINVAL and last() == "tf_build_eri: call tf_set_basis first"
            a, b_, s = ctypes.c_int32(7), ctypes.c_int32(7), ctypes.c_int32(7)
            assert L.tf_dims(ctx, a, b_, s) == EINVAL and (a.value, b_.value, s.value) == (7, 7, 7)
            assert last() == "tf_build_eri: call tf_set_basis first"      # (tf_dims leaves no text of its own)

        off_axis = np.array(good[0], dtype=np.float64, copy=True).reshape(-1, 3)
        off_axis[-1, 0] = 0.25
        off_axis = np.ascontiguousarray(off_axis)
        n = bases[1].n
        assert L.tf_set_basis(ctx, n, ptr(off_axis), ptr(good[1]), ptr(good[2]), ptr(good[3]), ptr(good[4])) == EGEOM
        assert last() == "Molecule is incorrectly aligned! Unable to calculate molecular integrals."
        refused_everywhere()
        assert L.tf_set_basis(ctx, n, None, ptr(good[1]), ptr(good[2]), ptr(good[3]), ptr(good[4])) == EINVAL
        assert last() == "tf_set_basis: null argument"
        refused_everywhere()
        with pytest.raises(TunaError):
            eng.copy_eri()
        assert np.array_equal(eng.set_basis(bases[1]).build_eri(True, "packed").copy_eri(), E_ref)
        for got, ref in zip(eng.one_electron(xyz, chg, org)[:3], STV_ref):
            assert np.array_equal(got, ref)
