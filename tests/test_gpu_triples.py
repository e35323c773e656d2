"""GPU: the perturbative triples of CCSD(T), QCISD(T) and full MP4 (tf_triples_rhf: rocBLAS for the six X_pqr of a triple, the fused
tftriples::triples_energy_kernel for W, V, D and the sums) against the reference program (tests/golden/triples_systems.npz) and, element
by element, the independent NumPy loop of tests/triples_reference.py on MO integrals that no library code made (mr.dense_eri +
mr.mo_tensor): random orthonormal orbitals, random non-symmetric t2 and random t1.

Bounds.  Goldens: 1e-10 for MP4 (the bound of the MP3 golden test), 1e-9 for the triples on amplitudes converged here (the bound of the
CCSD goldens for energies of converged amplitudes).  Element level: per ordered triple |e_ijk - ref| <= 1e-12 S_ijk, S_ijk = 1/3 sum
|(W + V) (...) / D| (the checker's sum of magnitudes), the same for both parts, and for the totals with S = sum S_ijk: the rounding model
(v + o) 2^-53 S gives 5e-14 S at v = 382 and less at the sizes here.  No case is left out of a comparison: every ordered triple of every
row is compared.  Every test hands the shared context back with the default layout."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import mp3_reference as mr
import triples_reference as tr
from test_ccd_reference import split
from test_gpu_ccd_large import _converged_orbitals
from test_gpu_ccsd import GOLD
from test_gpu_mp3 import SYSTEMS, _random_orbitals, _reset, _system
from tuna_amd._lib import TriplesResult, TunaError, ptr

pytestmark = pytest.mark.gpu

TF_EINVAL = -1
KINDS = ("CCSD(T)", "QCISD(T)", "MP4")
TAGS = ["n2_ccpvdz", "n2_ccpvtz", "co_631g", "hf_ccpvdz", "ne_ccpvdz"]


@pytest.fixture(scope="module")
def triples_golden(golden):
    return split(golden("triples_systems"))


@pytest.fixture(scope="module")
def mp3_golden(golden):
    return split(golden("mp3_systems"))


@pytest.fixture(scope="module")
def n2_tz():
    shells, aos = _system("n2_ccpvtz")
    return aos, mr.dense_eri(aos, shells)


@pytest.fixture(scope="module")
def n2_min():
    shells, aos = _system("n2_sto3g")
    return aos, mr.dense_eri(aos, shells)


class _Slab:
    """TF_TRIPLES_SLAB (occupied orbitals per slab) and TF_TRIPLES_SLICE (values of b per slice) of the (ia|bc) build for the duration of
    a with block (the library reads them per call).  Left alone, a call slices b only above N of about 240: the knob is the only way a
    test of these sizes reaches the strided copy of a slice into [i][a][b][c]."""
    KNOBS = ("TF_TRIPLES_SLAB", "TF_TRIPLES_SLICE")

    def __init__(self, slab=None, slice=None):
        self.want = dict(zip(self.KNOBS, (slab, slice)))

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in self.KNOBS}
        for k, n in self.want.items():
            if n is not None:
                os.environ[k] = str(n)

    def __exit__(self, *a):
        for k in self.KNOBS:
            os.environ.pop(k, None)
            if self.old[k] is not None:
                os.environ[k] = self.old[k]


def _amplitudes(o, v, seed):
    rng = np.random.default_rng(seed)
    return 0.1 * rng.standard_normal((o, v)), 0.1 * rng.standard_normal((o, o, v, v))          # t2 is NOT symmetric under (ij)(ab)


def _compare(r, ref, label, bad):
    """every ordered triple, both parts and the totals against the checker; returns the largest |d| / S seen"""
    o = ref["e_ijk"].shape[0]
    worst = 0.0
    for p in itertools.product(range(o), repeat=3):
        if p[0] == p[1] == p[2]:
            if r["e_ijk"][p] != 0.0:
                bad.append(f"{label}: e_{p} = {r['e_ijk'][p]!r} is not exactly 0.0")
            continue
        d, S = abs(r["e_ijk"][p] - ref["e_ijk"][p]), ref["S_ijk"][p]
        worst = max(worst, d / S)
        if not d <= 1e-12 * S:
            bad.append(f"{label}: e_{p} = {r['e_ijk'][p]!r}, reference {ref['e_ijk'][p]!r}, |d|/S = {d / S:.2e}")
    S = float(np.nansum(ref["S_ijk"]))
    for key in ("E_T", "E_connected", "E_disconnected"):
        d = abs(r[key] - ref[key])
        worst = max(worst, d / S)
        print(f"[{label}] {key} {r[key]:.12e} ref {ref[key]:.12e} |d|/S {d / S:.2e}")
        if not d <= 1e-12 * S:
            bad.append(f"{label}: {key} = {r[key]!r}, reference {ref[key]!r}, |d|/S = {d / S:.2e}")
    print(f"[{label}] worst |d|/S over the ordered triples, the parts and the totals {worst:.2e} (S {S:.3e})")
    return worst


def _off_diagonal(o):
    return [(i, j, k) for i in range(o) for j in range(i + 1) for k in range(j + 1) if i != k]


def _element_level(engine, E, C, eps, o, label, kinds=KINDS, seed=5):
    N = engine.N
    v = N - o
    Co, Cv, eo, ev = mr._windows(C, eps, o, 0)
    ovov, ovvv, ovoo = mr.mo_tensor(E, Co, Cv, Co, Cv), mr.mo_tensor(E, Co, Cv, Cv, Cv), mr.mo_tensor(E, Co, Cv, Co, Co)
    t1, t2 = _amplitudes(o, v, seed)
    bad = []
    for kind in kinds:
        amps = {} if kind == "MP4" else dict(t1=t1, t2=t2)
        r = engine.triples_rhf(C, eps, o, 0, kind=kind, return_e_ijk=True, **amps)
        ref = tr.triples(eo, ev, ovov, ovvv, ovoo, kind, only=_off_diagonal(o), **amps)
        print()
        _compare(r, ref, f"{label} {kind}", bad)
        assert r["n_triples"] == o * (o + 1) * (o + 2) // 6 - o and r["E_T"] == r["E_connected"] + r["E_disconnected"]
        assert (kind != "MP4") or r["E_disconnected"] == 0.0
        for s in itertools.permutations(range(3)):
            assert np.array_equal(r["e_ijk"], r["e_ijk"].transpose(s))
        assert abs(r["e_ijk"].sum() - r["E_T"]) <= 1e-13 * np.abs(r["e_ijk"]).sum()
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("tag", TAGS)
def test_reference_orbitals_against_goldens(engine, triples_golden, mp3_golden, tag):
    g, m = triples_golden[tag], mp3_golden[tag]
    engine.set_basis(_system(tag)[1]).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed"
    nocc = int(m["n_occ"])
    for nf in (0, 1):
        o = nocc - nf
        r = engine.triples_rhf(m["C"], m["eps"], nocc, nf, kind="MP4")
        want = float(g[f"MP4_fc{nf}_E_T"])
        print(f"\n[{tag} fc{nf}] MP4 E_T {r['E_T']:.12f} golden {want:.12f} d {r['E_T'] - want:.1e} seconds {r['seconds']}")
        assert abs(r["E_T"] - want) < 1e-10
        assert r["E_disconnected"] == 0.0 and r["E_T"] == r["E_connected"] + r["E_disconnected"]
        assert r["n_triples"] == o * (o + 1) * (o + 2) // 6 - o
        for method in ("CCSD", "QCISD"):
            cc = engine.ccsd_rhf(m["C"], m["eps"], nocc, nf, method=method, return_t1=True, return_t2=True, **GOLD)
            r = engine.triples_rhf(m["C"], m["eps"], nocc, nf, kind=f"{method}(T)", t1=cc["t1"], t2=cc["t2"])
            want = float(g[f"{method}_fc{nf}_E_T"])
            print(f"[{tag} fc{nf}] {method}(T) E_T {r['E_T']:.12f} golden {want:.12f} d {r['E_T'] - want:.1e} connected {r['E_connected']:.12f} "
                  f"disconnected {r['E_disconnected']:.12f}")
            assert abs(r["E_T"] - want) < 1e-9
            assert r["E_T"] == r["E_connected"] + r["E_disconnected"] and r["n_triples"] == o * (o + 1) * (o + 2) // 6 - o


def test_golden_file_holds_the_systems_and_amplitudes(triples_golden):
    assert set(triples_golden) == set(TAGS) <= set(SYSTEMS)
    for tag, g in triples_golden.items():
        for nf in (0, 1):
            assert all(f"{k}_fc{nf}_E_T" in g for k in ("MP4", "CCSD", "QCISD"))
        assert ("CCSD_fc0_t2" in g) == (tag in ("co_631g", "ne_ccpvdz"))


@pytest.mark.parametrize("width", [1, 2, 3, 7, 12])
def test_widths_against_the_independent_checker(engine, n2_tz, width):
    """N2/cc-pVTZ (N = 60), random orthonormal orbitals, v = 59, 58, 57, 53, 48: o = 1 (no triple); o = 2 (only i = j != k type triples);
    o = 3 (the first i > j > k); v = 53 (a ragged last tile of 5); v = 48 (whole tiles only)."""
    aos, E = n2_tz
    engine.set_basis(aos).build_eri(True)
    C, eps = _random_orbitals(engine.N, 30 + width)
    if width > 1:
        _element_level(engine, E, C, eps, width, f"width {width}")
        return
    # o = 1: the only triple is i = j = k, which the library skips: nothing runs beyond the MO blocks and every output is exactly 0.0,
    # inside the bound 1e-15 sum |X|^2 / min |D| that rounding noise of an evaluated e_000 would have to meet
    Co, Cv, eo, ev = mr._windows(C, eps, 1, 0)
    ovvv, ovoo = mr.mo_tensor(E, Co, Cv, Cv, Cv), mr.mo_tensor(E, Co, Cv, Co, Co)
    t1, t2 = _amplitudes(1, engine.N - 1, 5)
    X = tr._x(ovvv, ovoo, t2, 0, 0, 0)
    bound = 1e-15 * float((X * X).sum()) / abs(3.0 * eo[0] - 3.0 * ev[0])
    for kind in KINDS:
        amps = {} if kind == "MP4" else dict(t1=t1, t2=t2)
        r = engine.triples_rhf(C, eps, 1, 0, kind=kind, return_e_ijk=True, **amps)
        print(f"\n[width 1 {kind}] E_T {r['E_T']!r} e_000 {r['e_ijk'][0, 0, 0]!r} bound {bound:.2e} seconds {r['seconds']}")
        assert abs(r["E_T"]) <= bound and abs(r["e_ijk"][0, 0, 0]) <= bound and r["E_T"] == 0.0
        # the loop's share of the call (from the last stamp in front of it to the read-back behind it) is two clock reads and a
        # synchronisation of an idle device: microseconds.  One GEMM pair and one kernel launch would already be tens of microseconds
        # and a read-back; a millisecond separates the two by a wide margin on either side
        assert r["seconds"][2] < 1e-3 and r["seconds"][2] < 0.1 * r["seconds"][1]
        assert r["n_triples"] == 0 and r["e_ijk"].shape == (1, 1, 1)


@pytest.mark.parametrize("o", [7, 8, 9])
def test_small_virtual_spaces(engine, n2_min, o):
    """N2/STO-3G (N = 10): v = 3 (less than a tile), v = 2, v = 1"""
    aos, E = n2_min
    engine.set_basis(aos).build_eri(True)
    N = engine.N
    C = np.linalg.qr(np.random.default_rng(40 + o).standard_normal((N, N)))[0]
    eps = np.concatenate([-np.linspace(20.0, 11.0, o), np.linspace(0.3, 2.0, N - o)])
    if N - o > 1:
        _element_level(engine, E, C, eps, o, f"o {o} v {N - o}")
        return
    # v = 1: W^aaa is one number per triple and the bracket is formed as the four differences 2 (W - W^cba) + 2 (W - W^acb) +
    # (W^bca - W^bac) + (W^cab - W^bac) of the six slots, which hold that number computed by the same six additions in the same order:
    # every difference is exactly 0, so E_T is exactly 0.0 (not merely small)
    t1, t2 = _amplitudes(o, 1, 5)
    for kind in KINDS:
        amps = {} if kind == "MP4" else dict(t1=t1, t2=t2)
        r = engine.triples_rhf(C, eps, o, 0, kind=kind, return_e_ijk=True, **amps)
        print(f"\n[o 9 v 1 {kind}] E_T {r['E_T']!r} max |e_ijk| {np.abs(r['e_ijk']).max()!r}")
        assert r["E_T"] == 0.0 and r["E_connected"] == 0.0 and r["E_disconnected"] == 0.0 and not r["e_ijk"].any()
        assert r["n_triples"] == o * (o + 1) * (o + 2) // 6 - o


def test_kinds_slabs_and_repeatability(engine, n2_tz, mp3_golden):
    """the same (t1, t2) through kinds 0 and 1; t1 = 0; TF_TRIPLES_SLAB = 1, 2 (o = 7: a ragged last slab) and unset; two identical calls;
    TF_TRIPLES_SLICE = 5 (v = 53: ten slices and a last one of 3) and 16 (three and one of 5), alone and with slabs of 2: every ordered
    triple against the checker at 1e-12 S, like the unsliced call.  A slice changes the ket width of the transformation's GEMMs, so
    (ia|bc) and the energies differ from the unsliced call in the last bits (printed); the same slicing twice is bit-identical"""
    aos, E = n2_tz
    engine.set_basis(aos).build_eri(True)
    o, N = 7, engine.N
    C, eps = _random_orbitals(N, 37)
    t1, t2 = _amplitudes(o, N - o, 11)
    a = engine.triples_rhf(C, eps, o, 0, kind="CCSD(T)", t1=t1, t2=t2, return_e_ijk=True)
    q = engine.triples_rhf(C, eps, o, 0, kind="QCISD(T)", t1=t1, t2=t2, return_e_ijk=True)
    assert a["E_connected"] == q["E_connected"] and a["E_disconnected"] != 0.0
    assert abs(q["E_disconnected"] - 2.0 * a["E_disconnected"]) <= 4 * 2.0 ** -53 * abs(q["E_disconnected"])
    z = engine.triples_rhf(C, eps, o, 0, kind="CCSD(T)", t1=np.zeros_like(t1), t2=t2)
    assert z["E_disconnected"] == 0.0 and z["E_connected"] == a["E_connected"] and z["E_T"] == z["E_connected"]
    for kind, first in (("CCSD(T)", a), ("QCISD(T)", q)):
        again = engine.triples_rhf(C, eps, o, 0, kind=kind, t1=t1, t2=t2, return_e_ijk=True)
        assert all(again[k] == first[k] for k in ("E_T", "E_connected", "E_disconnected", "n_triples")) and np.array_equal(again["e_ijk"], first["e_ijk"])
    m4 = engine.triples_rhf(C, eps, o, 0, kind="MP4", return_e_ijk=True)
    for n in (1, 2):
        with _Slab(n):
            s = engine.triples_rhf(C, eps, o, 0, kind="CCSD(T)", t1=t1, t2=t2, return_e_ijk=True)
            s4 = engine.triples_rhf(C, eps, o, 0, kind="MP4", return_e_ijk=True)
        assert s["E_T"] == a["E_T"] and s["E_connected"] == a["E_connected"] and np.array_equal(s["e_ijk"], a["e_ijk"]), n
        assert s4["E_T"] == m4["E_T"] and np.array_equal(s4["e_ijk"], m4["e_ijk"]), n
    Co, Cv, eo, ev = mr._windows(C, eps, o, 0)
    blocks = mr.mo_tensor(E, Co, Cv, Co, Cv), mr.mo_tensor(E, Co, Cv, Cv, Cv), mr.mo_tensor(E, Co, Cv, Co, Co)
    ref = {"CCSD(T)": tr.triples(eo, ev, *blocks, "CCSD(T)", t1=t1, t2=t2, only=_off_diagonal(o)),
           "MP4": tr.triples(eo, ev, *blocks, "MP4", only=_off_diagonal(o))}
    bad = []
    print()
    _compare(a, ref["CCSD(T)"], "o 7 v 53 unsliced CCSD(T)", bad)
    for slab, sl in ((None, 5), (None, 16), (2, 5), (2, 16)):
        with _Slab(slab, sl):
            s = engine.triples_rhf(C, eps, o, 0, kind="CCSD(T)", t1=t1, t2=t2, return_e_ijk=True)
            s4 = engine.triples_rhf(C, eps, o, 0, kind="MP4", return_e_ijk=True)
            again = engine.triples_rhf(C, eps, o, 0, kind="CCSD(T)", t1=t1, t2=t2, return_e_ijk=True)
        same = s["E_T"] == a["E_T"] and np.array_equal(s["e_ijk"], a["e_ijk"]) and s4["E_T"] == m4["E_T"] and np.array_equal(s4["e_ijk"], m4["e_ijk"])
        print(f"[slab {slab} slice {sl}] bit-identical to the unsliced call: {same}")
        _compare(s, ref["CCSD(T)"], f"o 7 v 53 slab {slab} slice {sl} CCSD(T)", bad)
        _compare(s4, ref["MP4"], f"o 7 v 53 slab {slab} slice {sl} MP4", bad)
        assert again["E_T"] == s["E_T"] and np.array_equal(again["e_ijk"], s["e_ijk"]) and s["n_triples"] == a["n_triples"]
    assert not bad, "\n".join(bad[:20])
    assert not any(k in os.environ for k in _Slab.KNOBS)


def test_layouts_agree(engine, mp3_golden):
    """packed, tiles and rows at N2/cc-pVDZ within 1e-12 S, S from the checker on the packed layout's own MO blocks"""
    m = mp3_golden["n2_ccpvdz"]
    aos = _system("n2_ccpvdz")[1]
    C, eps, o = m["C"], m["eps"], 7
    try:
        e = {}
        for layout in ("packed", "tiles", "rows"):
            engine.set_basis(aos).build_eri(True, layout=layout)
            assert engine.eri_storage()["layout"] == layout
            t1, t2 = _amplitudes(o, engine.N - o, 3)
            e[layout] = {kind: engine.triples_rhf(C, eps, o, 0, kind=kind, return_e_ijk=True, **({} if kind == "MP4" else dict(t1=t1, t2=t2)))
                         for kind in KINDS}
            if layout == "packed":
                Co, Cv = np.ascontiguousarray(C[:, :o]), np.ascontiguousarray(C[:, o:])
                blocks = engine.ao_to_mo(Co, Cv, Co, Cv), engine.ao_to_mo(Co, Cv, Cv, Cv), engine.ao_to_mo(Co, Cv, Co, Co)
                S = {kind: tr.triples(eps[:o], eps[o:], *blocks, kind, only=_off_diagonal(o), **({} if kind == "MP4" else dict(t1=t1, t2=t2)))
                     for kind in KINDS}
        for kind in KINDS:
            Sk = S[kind]["S_ijk"]
            d0 = abs(e["packed"][kind]["E_T"] - S[kind]["E_T"]) / np.nansum(Sk)
            print(f"\n[{kind}] packed against the checker on the library's blocks |d|/S {d0:.1e}")
            assert d0 <= 1e-12
            for lt in ("tiles", "rows"):
                d = abs(e[lt][kind]["E_T"] - e["packed"][kind]["E_T"]) / np.nansum(Sk)
                off = ~np.isnan(Sk)
                dm = (np.abs(e[lt][kind]["e_ijk"] - e["packed"][kind]["e_ijk"])[off] / Sk[off]).max()
                print(f"[{kind}] {lt} - packed: E_T |d|/S {d:.1e}, worst e_ijk |d|/S_ijk {dm:.1e}")
                assert d <= 1e-12 and dm <= 1e-12
    finally:
        _reset(engine)
    engine.set_basis(aos).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed"


def test_the_other_methods_do_not_move(engine, mp3_golden):
    m = mp3_golden["n2_ccpvdz"]
    engine.set_basis(_system("n2_ccpvdz")[1]).build_eri(True)

    def others():
        r2, r3 = engine.mp2_rhf(m["C"], m["eps"], 7, 0), engine.mp3_rhf(m["C"], m["eps"], 7, 0)
        cc = engine.ccsd_rhf(m["C"], m["eps"], 7, 0, method="CCSD", return_t1=True, return_t2=True, **GOLD)
        return ([r2[k] for k in ("E_OS", "E_SS")], [r3[k] for k in ("E_OS", "E_SS", "E_pp", "E_hh", "E_ring")],
                (cc["E_corr"], cc["n_iter"], cc["table"].tobytes(), cc["t1"].tobytes(), cc["t2"].tobytes())), cc
    before, cc = others()
    for kind in KINDS:
        engine.triples_rhf(m["C"], m["eps"], 7, 0, kind=kind, **({} if kind == "MP4" else dict(t1=cc["t1"], t2=cc["t2"])))
    assert others()[0] == before


def test_mid_size_with_slabs(engine):
    """synthetic N = 120, converged RHF orbitals, o = 18 with 10 frozen (o = 8, v = 102: 13 tiles a side, the last of 6; the 120 unordered
    triples i >= j >= k less the 8 with i = j = k, 455 workgroups each), TF_TRIPLES_SLAB = 3 (slabs of 3, 3, 2) and TF_TRIPLES_SLICE = 40 (slices of 40, 40, 22): every ordered
    triple against the checker on the MO blocks of engine.ao_to_mo.  The CPU side takes about 5 s, so N stays at 120."""
    try:
        aos, C, eps, nocc = _converged_orbitals(engine, 120)
        nf = 10
        o, v = nocc - nf, engine.N - nocc
        assert engine.N == 120 and o == 8
        Co, Cv = np.ascontiguousarray(C[:, nf:nocc]), np.ascontiguousarray(C[:, nocc:])
        blocks = engine.ao_to_mo(Co, Cv, Co, Cv), engine.ao_to_mo(Co, Cv, Cv, Cv), engine.ao_to_mo(Co, Cv, Co, Co)
        t1, t2 = _amplitudes(o, v, 9)
        ref = tr.triples(eps[nf:nocc], eps[nocc:], *blocks, "CCSD(T)", t1=t1, t2=t2, only=_off_diagonal(o))
        with _Slab(3, 40):
            r = engine.triples_rhf(C, eps, nocc, nf, kind="CCSD(T)", t1=t1, t2=t2, return_e_ijk=True)
        print(f"\n[synth-120, 10 frozen] seconds {r['seconds']}")
        bad = []
        _compare(r, ref, "synth-120 o 8 v 102 slab 3 slice 40 CCSD(T)", bad)
        assert r["n_triples"] == 112 and not bad, "\n".join(bad[:20])
    finally:
        _reset(engine)


def test_refusals(engine, mp3_golden):
    from tuna_amd.engine import Engine
    m = mp3_golden["n2_ccpvdz"]
    shells, aos = _system("n2_ccpvdz")
    engine.set_basis(aos).build_eri(True)
    L, ctx, N = engine._L, engine._ctx, engine.N
    C, eps = (np.ascontiguousarray(x, dtype=np.float64) for x in (m["C"], m["eps"]))
    t1, t2 = _amplitudes(7, N - 7, 1)
    first = engine.triples_rhf(C, eps, 7, 0, kind="CCSD(T)", t1=t1, t2=t2)
    res = TriplesResult()
    pr, a1, a2 = ctypes.byref(res), ptr(t1), ptr(t2)
    bad = [(0, 7, -1, ptr(C), ptr(eps), a1, a2, pr), (0, 7, 7, ptr(C), ptr(eps), a1, a2, pr), (0, 0, 0, ptr(C), ptr(eps), a1, a2, pr),
           (0, N, 0, ptr(C), ptr(eps), a1, a2, pr), (0, 7, 0, None, ptr(eps), a1, a2, pr), (0, 7, 0, ptr(C), None, a1, a2, pr),
           (0, 7, 0, ptr(C), ptr(eps), a1, a2, None), (3, 7, 0, ptr(C), ptr(eps), a1, a2, pr), (-1, 7, 0, ptr(C), ptr(eps), a1, a2, pr),
           (0, 7, 0, ptr(C), ptr(eps), None, a2, pr), (1, 7, 0, ptr(C), ptr(eps), a1, None, pr), (2, 7, 0, ptr(C), ptr(eps), a1, None, pr),
           (2, 7, 0, ptr(C), ptr(eps), None, a2, pr)]
    for args in bad:
        assert L.tf_triples_rhf(ctx, *args) == TF_EINVAL, args
        again = engine.triples_rhf(C, eps, 7, 0, kind="CCSD(T)", t1=t1, t2=t2)            # the context stays usable
        assert again["E_T"] == first["E_T"]
    assert L.tf_triples_rhf(None, 0, 7, 0, ptr(C), ptr(eps), a1, a2, pr) == TF_EINVAL
    with Engine(0) as fresh:                                          # no tensor yet
        fresh.set_basis(aos)
        assert fresh._L.tf_triples_rhf(fresh._ctx, 0, 7, 0, ptr(C), ptr(eps), a1, a2, pr) == TF_EINVAL
    with Engine(0, 0, 2) as half:                                     # rank 0 of two: sharding is not supported
        half.set_basis(aos).build_eri(True)
        assert half._L.tf_triples_rhf(half._ctx, 0, 7, 0, ptr(C), ptr(eps), a1, a2, pr) == TF_EINVAL
    for kw in (dict(kind="CCSD"), dict(kind="MP4", t1=t1), dict(kind="CCSD(T)", t1=t1), dict(kind="QCISD(T)", t1=t1, t2=t2[:, :, :, 1:]),
               dict(kind="CCSD(T)", t1=t1[1:], t2=t2)):
        with pytest.raises(TunaError):
            engine.triples_rhf(C, eps, 7, 0, **kw)
    with pytest.raises(TunaError):
        engine.mp4_rhf(C, eps, 7, 0, level="SDTQ")
    with pytest.raises(TunaError):
        engine.ccsd_rhf(C, eps, 7, 0, method="CCSD(T)")
    assert engine.triples_rhf(C, eps, 7, 0, kind="CCSD(T)", t1=t1, t2=t2)["E_T"] == first["E_T"]
    assert engine.eri_storage()["layout"] == "packed"


def test_energy_driver(engine, triples_golden, mp3_golden, golden):
    """calculate_energy with a Calculation that names the method and triples (the input line does not route these names)"""
    from tuna_amd import energy
    g, E_SCF = triples_golden["n2_ccpvdz"], float(mp3_golden["n2_ccpvdz"]["E_SCF"])
    g4 = split(golden("mp4_systems"))["n2_ccpvdz"]
    _, _, basis, symbols, R, params = energy.parse_input("SPE : N N 1.0977 : HF CC-PVDZ : TIGHT")
    for method in ("CCSD", "QCISD"):
        calc = energy.interpret_keywords(params, energy.Calculation("SPE", "HF", basis))
        calc.coupled_cluster, calc.triples = method, True
        log = []
        out = energy.calculate_energy(symbols, R, calc, engine, False, log.append)
        want = E_SCF + float(g[f"{method}_fc0_E_corr"]) + float(g[f"{method}_fc0_E_T"])
        print(f"\n[{method}(T)] E = {out.energy:.10f} (golden {want:.10f}, d {out.energy - want:.1e}) E_T {out.correlation_energy_triples:.10f}")
        assert abs(out.energy - want) < 1e-8, (method, out.energy, want)
        assert out.correlation_energy_triples == out.triples["E_T"] and out.correlation_energy_cc == out.cc["E_corr"]
        text = "\n".join(log)
        for s in (f"                    {method}(T) Energy ", "  Forming disconnected amplitudes...         [Done]",
                  "  Forming connected amplitudes...            [Done]", f"  {method}(T) correlation energy:       ",
                  f" Correlation energy from {method}:", f" Correlation energy from {method}(T):", " Final single point energy:"):
            assert s in text, s
        assert text.index(f" Correlation energy from {method}:") < text.index(f"                    {method}(T) Energy ")
    calc = energy.interpret_keywords(params, energy.Calculation("SPE", "MP2", basis))
    calc.mp4 = "SDTQ"
    log = []
    out = energy.calculate_energy(symbols, R, calc, engine, False, log.append)
    parts = [float(g4["SDQ_fc0_E_S"]), float(g4["SDQ_fc0_E_D"]), float(g["MP4_fc0_E_T"]), float(g4["SDQ_fc0_E_Q"])]
    want = E_SCF + float(mp3_golden["n2_ccpvdz"]["E_OS"]) + float(mp3_golden["n2_ccpvdz"]["E_SS"]) + float(g4["fc0_E_MP3"]) + sum(parts)
    print(f"\n[MP4] E = {out.energy:.10f} (golden {want:.10f}, d {out.energy - want:.1e})")
    assert abs(out.energy - want) < 1e-8
    assert abs(out.correlation_energy_mp4 - sum(parts)) < 1e-9 and out.mp4["E_T"] == out.triples["E_T"]
    text = "\n".join(log)
    for s in ("  Triples are included in full MP4.\n", f"  Triples correlation energy:         {out.triples['E_T']:13.10f}",
              " Correlation energy from MP4:      "):
        assert s in text, s
    with pytest.raises(TunaError, match="is not supported"):
        energy.run("SPE : N N 1.0977 : CCSD(T) STO-3G", engine=engine)
