"""GPU: restricted MP4(SDQ) / MP4(DQ) on the resident tensor (tf_mp4_rhf) against the reference program's run_restricted_MP4
(tests/golden/mp4_systems.npz) and the independent NumPy MP4 of tests/mp4_reference.py; the MP2 and MP3 parts bit for bit against
tf_mp3_rhf; E_D and E_Q against the step differences of tf_ccd_rhf (other code of the library); the layouts against each other;
repeatability; refusals; the input lines of energy.run.  Every test hands the shared context back with the default layout."""
import ctypes

import numpy as np
import pytest

import mp3_reference as mr
import mp4_reference as m4
from test_ccd_reference import split
from test_gpu_mp3 import SYSTEMS, _random_orbitals, _reset, _system
from tuna_amd._lib import TunaError, ptr

pytestmark = pytest.mark.gpu

TF_EINVAL = -1
PARTS = ("E_S", "E_D", "E_Q", "E_MP4")
MP3_KEYS = ("E_OS", "E_SS", "E_MP2", "E_pp", "E_hh", "E_ring", "E_MP3")


@pytest.fixture(scope="module")
def mp4_golden(golden):
    return split(golden("mp4_systems"))


@pytest.fixture(scope="module")
def mp3_golden(golden):
    return split(golden("mp3_systems"))


@pytest.fixture(scope="module")
def n2_tz():
    shells, aos = _system("n2_ccpvtz")
    return aos, mr.dense_eri(aos, shells)


@pytest.mark.parametrize("tag", list(SYSTEMS))
def test_reference_orbitals_against_goldens(engine, mp4_golden, mp3_golden, tag):
    g, m = mp4_golden[tag], mp3_golden[tag]
    engine.set_basis(_system(tag)[1]).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed"
    nocc = int(m["n_occ"])
    bad = []
    for nf in (0, 1):
        r3 = engine.mp3_rhf(m["C"], m["eps"], nocc, nf)
        for level in ("SDQ", "DQ"):
            r = engine.mp4_rhf(m["C"], m["eps"], nocc, nf, level=level)
            d = {k: r[k] - float(g[f"{level}_fc{nf}_{k}"]) for k in PARTS}
            print(f"\n[{tag} fc{nf} {level}] " + " ".join(f"{k} {r[k]:.12f} (d {d[k]:.1e})" for k in PARTS) + f" seconds {r['seconds']}")
            bad += [(nf, level, k, d[k]) for k in PARTS if not abs(d[k]) < 1e-10]
            assert r["E_MP4"] == r["E_S"] + r["E_D"] + r["E_Q"]
            assert level == "SDQ" or r["E_S"] == 0.0
            assert all(r[k] == r3[k] for k in MP3_KEYS), (r, r3)          # bit for bit tf_mp3_rhf
    assert not bad, bad


def test_doubles_and_quadruples_are_the_step_differences_of_ccd(engine, mp3_golden, n2_tz):
    """E_D = E[LCCD step 2] - E[LCCD step 1], E_Q = E[CCD step 1] - E[LCCD step 1], the steps by tf_ccd_rhf (its update kernel and its
    intermediates: none of tf_mp4_rhf's GEMMs); bound as test_gpu_ccd.py's test_lccd_step_one_is_mp2_plus_mp3 has it for a step energy"""
    m = mp3_golden["n2_ccpvtz"]
    engine.set_basis(n2_tz[0]).build_eri(True)
    for nf in (0, 1):
        r = engine.mp4_rhf(m["C"], m["eps"], 7, nf)
        lccd = engine.ccd_rhf(m["C"], m["eps"], 7, nf, method="LCCD", max_iter=2, use_diis=False, allow_unconverged=True)["table"]
        ccd = engine.ccd_rhf(m["C"], m["eps"], 7, nf, method="CCD", max_iter=1, use_diis=False, allow_unconverged=True)["table"]
        bound = 1e-11 * abs(r["E_MP2"] + r["E_MP3"])
        dD, dQ = r["E_D"] - (lccd[1, 1] - lccd[0, 1]), r["E_Q"] - (ccd[0, 1] - lccd[0, 1])
        print(f"\n[N2/cc-pVTZ fc{nf}] E_D {r['E_D']:.13f} d {dD:.1e}  E_Q {r['E_Q']:.13f} d {dQ:.1e}  bound {bound:.1e}")
        assert abs(dD) <= bound and abs(dQ) <= bound


@pytest.mark.parametrize("width", [1, 7, 8, 12])
def test_widths_against_the_independent_checker(engine, n2_tz, width):
    """N2/cc-pVTZ, random orthonormal orbitals: one pair; 49 pairs (one partial batch of the ladder); 64 pairs (one full batch); 144 pairs
    (three batches, the last one partial).  The checker's E_D and E_Q are differences of step energies, each rounded relative to the
    step energy: the bound is the one of a step energy, 1e-11 |E_MP2 + E_MP3|, for every component."""
    aos, E = n2_tz
    engine.set_basis(aos).build_eri(True)
    C, eps = _random_orbitals(engine.N, 30 + width)
    want = m4.components(E, C, eps, width, 0, form="restricted")
    bound = 1e-11 * abs(want["E_MP2"] + want["E_MP3"])
    for level in ("SDQ", "DQ"):
        r = engine.mp4_rhf(C, eps, width, 0, level=level)
        d = {k: r[k] - (0.0 if (level == "DQ" and k == "E_S") else want[k]) for k in ("E_S", "E_D", "E_Q")}
        print(f"\n[width {width} {level}] " + " ".join(f"{k} {r[k]:.12f} (d {d[k]:.1e})" for k in d) + f" bound {bound:.1e}")
        assert all(abs(x) <= bound for x in d.values()), (width, level, d, bound)
        assert level == "SDQ" or r["E_S"] == 0.0


def test_layouts_agree(engine, mp3_golden, n2_tz):
    """packed (the ladder kernel, both stored-triangle halves of the occupied rows) against rows and tiles (the exchange-build route)"""
    m = mp3_golden["n2_ccpvtz"]
    try:
        e = {}
        for layout in ("packed", "rows", "tiles"):
            engine.set_basis(n2_tz[0]).build_eri(True, layout=layout)
            assert engine.eri_storage()["layout"] == layout
            e[layout] = engine.mp4_rhf(m["C"], m["eps"], 7, 1)
        for lt in ("rows", "tiles"):
            rel = {k: abs(e[lt][k] - e["packed"][k]) / abs(e["packed"][k]) for k in ("E_S", "E_D", "E_Q")}
            print(f"\n[{lt} against packed] {rel}")
            assert all(x < 1e-12 for x in rel.values()), (lt, rel)
    finally:
        _reset(engine)
    engine.set_basis(n2_tz[0]).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed"


def test_repeatable_and_refusals(engine, mp4_golden, mp3_golden):
    from tuna_amd.engine import Engine
    g, m = mp4_golden["n2_ccpvdz"], mp3_golden["n2_ccpvdz"]
    shells, aos = _system("n2_ccpvdz")
    engine.set_basis(aos).build_eri(True)
    a, b = engine.mp4_rhf(m["C"], m["eps"], 7), engine.mp4_rhf(m["C"], m["eps"], 7)
    assert all(a[k] == b[k] for k in PARTS + MP3_KEYS)
    L, ctx, N = engine._L, engine._ctx, engine.N
    C, eps = (np.ascontiguousarray(x, dtype=np.float64) for x in (m["C"], m["eps"]))
    e2, e3, e4 = (ctypes.c_double * 2)(), (ctypes.c_double * 3)(), (ctypes.c_double * 3)()
    pC, pe = ptr(C), ptr(eps)
    bad = [(1, 7, -1, pC, pe, e2, e3, e4), (1, 7, 7, pC, pe, e2, e3, e4), (1, 0, 0, pC, pe, e2, e3, e4), (1, N, 0, pC, pe, e2, e3, e4),
           (1, 7, 0, None, pe, e2, e3, e4), (1, 7, 0, pC, None, e2, e3, e4), (1, 7, 0, pC, pe, None, e3, e4), (1, 7, 0, pC, pe, e2, None, e4),
           (1, 7, 0, pC, pe, e2, e3, None), (2, 7, 0, pC, pe, e2, e3, e4), (-1, 7, 0, pC, pe, e2, e3, e4)]
    for args in bad:
        assert L.tf_mp4_rhf(ctx, *args, None) == TF_EINVAL, args
        r = engine.mp4_rhf(m["C"], m["eps"], 7)                          # the context stays usable
        assert all(r[k] == a[k] for k in PARTS)
    assert L.tf_mp4_rhf(None, 1, 7, 0, pC, pe, e2, e3, e4, None) == TF_EINVAL
    with pytest.raises(TunaError):
        engine.mp4_rhf(m["C"], m["eps"], 7, level="SDTQ")
    with Engine(0) as fresh:                                          # no tensor yet
        fresh.set_basis(aos)
        assert fresh._L.tf_mp4_rhf(fresh._ctx, 1, 7, 0, pC, pe, e2, e3, e4, None) == TF_EINVAL
    with Engine(0, 0, 2) as half:                                     # rank 0 of two: sharding is not supported
        half.set_basis(aos).build_eri(True)
        assert half._L.tf_mp4_rhf(half._ctx, 1, 7, 0, pC, pe, e2, e3, e4, None) == TF_EINVAL
    r = engine.mp4_rhf(m["C"], m["eps"], 7)
    assert all(abs(r[k] - float(g[f"SDQ_fc0_{k}"])) < 1e-10 for k in PARTS)
    assert len(r["seconds"]) == 4 and r["seconds"][0] >= r["seconds"][1] + r["seconds"][2] > 0.0


def test_input_lines(engine, mp4_golden, mp3_golden):
    from tuna_amd.energy import run
    g, n2 = mp4_golden["n2_ccpvtz"], mp3_golden["n2_ccpvtz"]
    base = sum(float(n2[k]) for k in ("E_SCF", "E_OS", "E_SS", "E_MP3"))
    text = []
    for name, level in (("MP4(SDQ)", "SDQ"), ("MP4[SDQ]", "SDQ"), ("MP4(DQ)", "DQ"), ("MP4[DQ]", "DQ")):
        line, want = f"SPE : N N 1.0977 : {name} CC-PVTZ : EXTREME", base + sum(float(g[f"{level}_fc0_{k}"]) for k in ("E_S", "E_D", "E_Q"))
        log = []
        out = run(line, silent=False, engine=engine, log=log.append)
        print(f"\n[{line}] E = {out.energy:.10f} (golden {want:.10f}, d {out.energy - want:.1e})")
        assert abs(out.energy - want) < 1e-8, (line, out.energy, want)
        assert out.correlation_energy_mp4 == out.mp4["E_MP4"] and out.mp4["E_MP3"] == out.correlation_energy_mp3
        text += log
    text = "\n".join(text)
    for s in ("MP4 Energy", "Triples are not included in MP4(SDQ).", "Singles and triples are not included in MP4(DQ).",
              "Singles correlation energy:", "Doubles correlation energy:", "Triples correlation energy:          0.0000000000",
              "Quadruples correlation energy:", "MP4 correlation energy:", "Correlation energy from MP2:", "Correlation energy from MP3:",
              "Correlation energy from MP4(SDQ): ", "Correlation energy from MP4(DQ):  ", "Total correlation energy:", "MP3 correlation energy:",
              "Same spin contribution:", "Opposite spin contribution:", "MP2 correlation energy:"):
        assert s in text, s
    for line in ("SPE : O O 1.2075 : MP4(SDQ) STO-3G : ML 3", "SPE : N N 1.0977 : UMP4(SDQ) STO-3G", "SPE : N N 1.0977 : MP4(DQ) STO-3G : DIPOLE",
                 "SPE : N N 1.0977 : MP4 STO-3G", "SPE : N N 1.0977 : MP4[SDTQ] STO-3G"):
        with pytest.raises(TunaError):
            run(line, engine=engine)
