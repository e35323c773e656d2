"""CPU: the HIP-free parts of the context core, compiled with g++ through tests/ctx_model.

Owners (tuna_amd/csrc/tf_ctx_plan.h) against a runtime that counts and can refuse its k-th request: a grow-only block keeps what is large
enough and grows by free-then-allocate, `replace` always hands out a fresh block, a refused request leaves {nullptr, 0} and nothing
leaked; the stream / event set of the tensor build is made whole or not at all, and destroy() destroys every handle exactly once -- every
stream and event a context creates is destroyed with it.  The same checks run as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer where their runtime is installed.

Shard plans (tf_shard_plan.h): the owners equal those recorded from the library before the plans moved into the header
(tests/golden/shard_plans.json, tools/record_shard_plans.py), and every pair has one owner in [0, world).

Device tables (tf::build_device_tables, tf_host.cpp) against an independent NumPy computation written here."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import make_system
from tuna_amd import molecule as mol
from tuna_amd import spherical

HERE = os.path.dirname(os.path.abspath(__file__))
MODEL = os.path.join(HERE, "ctx_model")
CSRC = os.path.join(HERE, "..", "tuna_amd", "csrc")
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(MODEL, "_build", "libctxmodel.so")
        src = [os.path.join(MODEL, f) for f in ("ctx_model.cpp", "owner_checks.h", "owner_main.cpp", "build.sh")]
        src += [os.path.join(CSRC, f) for f in ("tf_ctx_plan.h", "tf_eigh_plan.h", "tf_shard_plan.h", "tf_packed.h", "tf_host.cpp", "tf_internal.h", "tf_eri_types.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
            subprocess.check_call(["sh", os.path.join(MODEL, "build.sh")])
        L = C.CDLL(so)
        vp, ci = C.c_void_p, C.c_int
        L.ctxm_counts.argtypes = [vp]
        L.ctxm_block_growth.argtypes = [ci]
        L.ctxm_block_refusal.argtypes = [ci, ci, ci]
        L.ctxm_streams.argtypes = [ci, vp]
        L.ctxm_streams_verdict.argtypes = [ci, vp]
        L.ctxm_event_pairs.argtypes = [ci, ci]
        L.ctxm_shard_plan_pairs.argtypes = [ci, vp, ci, ci, ci, vp]
        L.ctxm_shard_plan.argtypes = [ci, vp, ci, vp]
        L.ctxm_tables.restype = vp
        L.ctxm_tables.argtypes = [ci, vp, vp, vp, vp, vp, ci]
        L.ctxm_tables_free.argtypes = [vp]
        L.ctxm_tables_sizes.argtypes = [vp, vp]
        L.ctxm_tables_copy.argtypes = [vp, ci, vp]
        _LIB = L
    return _LIB


def counts():
    out = np.zeros(3, dtype=np.int64)
    lib().ctxm_counts(out.ctypes.data)
    return [int(x) for x in out]                  # context blocks, streams of the build, events of the build


# ---- owners ---------------------------------------------------------------------------------------------------------------------

def test_headers_include_no_hip():
    for name in ("tf_ctx_plan.h", "tf_shard_plan.h", "tf_eri_types.h", "tf_packed.h"):
        with open(os.path.join(CSRC, name)) as f:
            assert "hip_runtime" not in f.read(), name


def test_blocks_grow_replace_and_release():
    n_blocks = counts()[0]
    assert n_blocks >= 12
    for slot in range(n_blocks):
        assert lib().ctxm_block_growth(slot) == 0, slot


def test_a_refused_block_leaves_an_empty_slot_and_no_leak():
    n_blocks = counts()[0]
    for k in range(-1, n_blocks):
        for grow in (0, 1):
            for use_replace in (0, 1):
                assert lib().ctxm_block_refusal(k, grow, use_replace) == 0, (k, grow, use_replace)


def test_stream_set_is_made_whole_or_not_at_all_and_destroyed_once():
    _, n_streams, n_events = counts()
    n = n_streams + n_events
    assert n_streams >= 9 and n_events >= 12      # eight build streams and their events, the list stream, two slab event pairs
    refused = lib().ctxm_refused()
    for k in range(-1, n):
        o = np.zeros(13, dtype=np.int64)
        lib().ctxm_streams(k, o.ctypes.data)
        assert lib().ctxm_streams_verdict(k, o.ctypes.data) == 0, (k, o.tolist())
        if k < 0:                                 # the full set: every handle made is destroyed exactly once by destroy()
            assert o.tolist() == [0, n, n, 1, n, n, n, 0, 0, 0, 0, n, 0]
        else:                                     # refused at k: create() itself destroyed the k handles it had made
            assert o.tolist() == [refused, k + 1, k, 0, 0, 0, k, 0, 0, 0, 0, k, 0]
    assert lib().ctxm_streams_names() == 0


def test_profile_event_pairs():
    for k in range(-1, 8):
        assert lib().ctxm_event_pairs(4, k) == 0, k


def test_owner_checks_as_a_sanitized_program():
    """tests/ctx_model/owner_main.cpp: with -fsanitize=address,undefined where build.sh found the runtime"""
    lib()
    exe = os.path.join(MODEL, "_build", "owner_main")
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout, p.stderr, "sanitized" if os.path.exists(exe + ".sanitized") else "built without the sanitizers")
    assert p.returncode == 0 and "0 failed" in p.stdout


# ---- shard plans ----------------------------------------------------------------------------------------------------------------

with open(os.path.join(HERE, "golden", "shard_plans.json")) as _f:
    PLANS = json.load(_f)


def _owners(s):
    """a recorded array: "rank x count" runs in order"""
    runs = [t.split("x") for t in s.split()]
    return np.repeat(np.array([int(r) for r, _ in runs], dtype=np.int32), [int(n) for _, n in runs])


def _recorded(rec, forced, layout, world):
    s = rec["pairs"][f"{forced or 'auto'}/{layout}/{world}"]
    return _owners(rec["pairs"][f"{s}/{layout}/{world}"] if s in ("segments", "shells") else s)     # (the free plan names the forced one it equals)


def test_shard_plan_cases_are_the_named_systems():
    cases = PLANS["cases"]
    for tag in ("n2_ccpvdz", "c3_ar2_ccpvqz"):
        assert cases[tag]["dim"] == [s.n_sph for s in make_system(tag)[1]]
    atoms = mol.make_atoms(["AR", "AR"], 7.1)
    shells = mol.build_shells(atoms, {18: mol.even_tempered_basis(*mol.synthetic_counts(400))})
    assert cases["synthetic_400"]["dim"] == [s.n_sph for s in shells] and sum(cases["synthetic_400"]["dim"]) == 400
    assert len(cases["one_shell"]["dim"]) == 1 and len(set(cases["all_equal"]["dim"])) == 1
    d = cases["one_heavy"]["dim"]
    assert max(d) > sum(d) - max(d)
    assert PLANS["worlds"] == [1, 2, 3, 4, 8] and PLANS["forced"] == ["", "segments", "shells"]


@pytest.mark.parametrize("name", sorted(PLANS["cases"]))
def test_shard_plans_equal_the_recorded_owners(name):
    rec = PLANS["cases"][name]
    dim = np.asarray(rec["dim"], dtype=np.int32)
    ns = len(dim)
    seen = 0
    for fi, forced in enumerate(PLANS["forced"]):
        for layout in (0, 1):
            for world in PLANS["worlds"]:
                owner = np.full(ns * (ns + 1) // 2, -1, dtype=np.int32)
                lib().ctxm_shard_plan_pairs(ns, dim.ctypes.data, layout, world, fi, owner.ctypes.data)
                assert owner.min() >= 0 and owner.max() < world                 # every pair has one owner in [0, world)
                assert np.array_equal(owner, _recorded(rec, forced, layout, world)), (forced, layout, world)
                seen += 1
    assert seen == len(rec["pairs"]) == 30
    w = dim.astype(np.int64) ** 2
    for world in PLANS["worlds"]:
        owner = np.full(ns, -1, dtype=np.int32)
        lib().ctxm_shard_plan(ns, w.ctypes.data, world, owner.ctypes.data)
        assert owner.min() >= 0 and owner.max() < world
        assert np.array_equal(owner, _owners(rec["lpt"][str(world)])), world


# ---- device tables --------------------------------------------------------------------------------------------------------------

def _tables(aos, exact):
    L = lib()
    o, l, p = np.ascontiguousarray(aos.origin, dtype=np.float64), np.ascontiguousarray(aos.lmn, dtype=np.int32), np.ascontiguousarray(aos.prim_off, dtype=np.int32)
    e, c = np.ascontiguousarray(aos.exps, dtype=np.float64), np.ascontiguousarray(aos.coefs, dtype=np.float64)
    h = L.ctxm_tables(aos.n, o.ctypes.data, l.ctypes.data, p.ctypes.data, e.ctypes.data, c.ctypes.data, int(exact))
    assert h
    try:
        sz = np.zeros(11, dtype=np.int64)
        L.ctxm_tables_sizes(h, sz.ctypes.data)
        ns, npair, nct, ncls, ncomp, nbase, nptr, nidx, npos, nord, nsc = (int(x) for x in sz)
        assert nct == npos == nord == nsc

        def get(which, shape, dtype=np.int32):
            a = np.zeros(shape, dtype=dtype)
            L.ctxm_tables_copy(h, which, a.ctypes.data)
            return a
        return dict(shells=get(0, (ns, 5)), pairs=get(1, (npair, 18)), pair_class=get(2, npair), class_pairs=get(3, (npair, 2)), ct_ix=get(4, nct),
                    ct_pos=get(5, nct), ct_ord=get(6, nct), sph_base=get(7, nbase), sph_ptr=get(8, nptr), sph_idx=get(9, nidx), comps=get(10, (ncomp, 3)),
                    ct_sc=get(20, nct, np.float64), sph_val=get(21, nidx, np.float64), c_scale=get(22, ncomp, np.float64), n_classes=ncls)
    finally:
        L.ctxm_tables_free(h)


def _basis_case(case):
    if case == "n2_ccpvtz":
        return make_system("c2_n2_ccpvtz")[2]
    if case == "g_and_h_shells":
        return make_system("high_l")[2]
    # the DECONTRACT ordering: per Cartesian component one AO per primitive, so no contiguous shells -- one-component shells
    atoms = mol.make_atoms(["N", "N"], mol.angstrom_to_bohr(1.0977))
    origin, lmn, exps = [], [], []
    for at in atoms:
        for letter, prims in mol.atomic_basis("6-31G*", 7):
            for comp in mol.cartesian_components(mol.SHELL_LETTERS.find(letter)):
                for e, _ in prims:
                    origin.append(at.origin); lmn.append(comp); exps.append(e)
    n = len(exps)
    return mol.AOList(np.array(origin, dtype=float), np.array(lmn, dtype=np.int32), np.ones(n, dtype=np.int32), np.arange(n + 1, dtype=np.int32),
                      np.array(exps), np.ones(n))


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("case", ["n2_ccpvtz", "g_and_h_shells", "decontract"])
def test_device_tables_against_numpy(case, exact):
    t = _tables(_basis_case(case), exact)
    shells, pairs, comps = t["shells"], t["pairs"], t["comps"]
    if case == "decontract":
        assert (shells[:, 4] == 0).any() and (shells[shells[:, 4] == 0, 1] == 1).all()      # one-component shells that are not complete
    if case == "g_and_h_shells":
        assert {4, 5} <= set(shells[:, 0].tolist())
    A, B, La, Lb, npp, cls, nca, ncb, coa, cob, _, _, tab_off = (pairs[:, k] for k in range(13))
    pcls = pairs[:, 13:18]
    assert np.array_equal(La, shells[A, 0]) and np.array_equal(Lb, shells[B, 0]) and np.array_equal(nca, shells[A, 1]) and np.array_equal(ncb, shells[B, 1])
    assert np.array_equal(coa, shells[A, 2]) and np.array_equal(cob, shells[B, 2])

    # two pairs share a class exactly when (La, Lb, depth, nca, ncb, component codes) agree
    def code(s):
        L_, nc, off, _, full = shells[s]
        return None if full else tuple(map(tuple, comps[off:off + min(nc, 2)]))
    keys = [(int(La[i]), int(Lb[i]), int(npp[i]) if exact else int(npp[i] == 1), int(nca[i]), int(ncb[i]), code(A[i]), code(B[i])) for i in range(len(pairs))]
    by_key, by_cls = {}, {}
    for i, k in enumerate(keys):
        assert by_key.setdefault(k, int(cls[i])) == int(cls[i])              # same key -> same class
        assert by_cls.setdefault(int(cls[i]), k) == k                        # same class -> same key
    assert np.array_equal(t["pair_class"], cls)
    assert sorted(by_cls) == list(range(t["n_classes"]))                    # ids are dense, in order of first appearance
    first = [int(np.nonzero(cls == c)[0][0]) for c in range(t["n_classes"])]
    assert first == sorted(first)
    # class_pairs is the ascending partition
    cp = t["class_pairs"]
    assert sorted(cp[:, 1].tolist()) == list(range(len(pairs)))
    for c in range(t["n_classes"]):
        members = cp[cp[:, 0] == c, 1]
        assert np.array_equal(members, np.nonzero(cls == c)[0])
    assert (np.diff(cp[:, 0]) >= 0).all()

    # component-pair tables
    off = 0
    for i in range(len(pairs)):
        nab, L2 = int(nca[i] * ncb[i]), int(Lb[i]) + 1
        assert tab_off[i] == off
        ca, cb = np.divmod(np.arange(nab), int(ncb[i]))
        u, w = comps[coa[i] + ca], comps[cob[i] + cb]
        par = ((u[:, 0] + w[:, 0]) & 1) | (((u[:, 1] + w[:, 1]) & 1) << 1)
        ix = t["ct_ix"][off:off + nab]
        for axis in range(3):                                                # each word decodes to the components' powers ...
            field = (ix >> (8 * axis)) & 0xff
            assert np.array_equal(field // L2, u[:, axis]) and np.array_equal(field % L2, w[:, axis])
        assert np.array_equal(ix >> 24, par)                                 # ... and parity
        assert np.array_equal(t["ct_pos"][off:off + nab], (ca << 8) | cb)
        assert np.array_equal(t["ct_sc"][off:off + nab], t["c_scale"][coa[i] + ca] * t["c_scale"][cob[i] + cb])     # the product of the two scales
        order = np.concatenate([np.nonzero(par == c)[0] for c in range(4)])   # class by class, ascending inside a class
        assert np.array_equal(t["ct_ord"][off:off + nab], order)
        assert pcls[i].tolist() == [0] + np.cumsum([int((par == c).sum()) for c in range(4)]).tolist()
        off += nab
    assert off == len(t["ct_ix"])

    # the per-L spherical CSR, rebuilt densely.  Both sides form an entry (magnitude below 4, one ulp 4.4e-16) from a handful of square
    # roots, factorials and binomials in double precision: they agree to a few ulp, 4e-15 at the most.  Exact zeros are not stored.
    base, ptr = t["sph_base"], t["sph_ptr"]
    assert len(base) == 7 and len(ptr) == sum(2 * L + 1 for L in range(6)) + 1
    for L in range(6):
        nc = (L + 1) * (L + 2) // 2
        dense = np.zeros((2 * L + 1, nc))
        for r in range(2 * L + 1):
            lo, hi = ptr[base[L] + r], ptr[base[L] + r + 1]
            assert (t["sph_val"][lo:hi] != 0).all() and (np.diff(t["sph_idx"][lo:hi]) > 0).all()
            dense[r, t["sph_idx"][lo:hi]] = t["sph_val"][lo:hi]
        ref = spherical.spherical_block(L)
        assert np.abs(ref).max() < 4.0
        np.testing.assert_allclose(dense, ref, atol=4e-15, rtol=0)
        assert np.array_equal(dense != 0, np.abs(ref) > 1e-12)
