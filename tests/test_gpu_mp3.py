"""GPU: restricted MP3 on the resident tensor (tf_mp3_rhf: the AO-direct ladder kernel tfmp3::mp3_ladder_kernel on the packed layout,
the general-density exchange build on the rows and tiles layouts) against the reference program's run_restricted_MP3
(tests/golden/mp3_systems.npz) and the independent NumPy MP3 of tests/mp3_reference.py; the MP2 part against tf_mp2_rhf; the layouts
against each other; repeatability; refusals; the input lines of energy.run.  Every test hands the shared context back with the default
layout."""
import numpy as np
import pytest

import mp3_reference as mr
from conftest import R_N2
from tuna_amd import molecule as mol
from tuna_amd._lib import TunaError

pytestmark = pytest.mark.gpu

TF_EINVAL = -1
SYSTEMS = {"n2_sto3g": (["N", "N"], R_N2, "STO-3G"), "n2_ccpvdz": (["N", "N"], R_N2, "cc-pVDZ"), "n2_ccpvtz": (["N", "N"], R_N2, "cc-pVTZ"),
           "co_631g": (["C", "O"], mol.angstrom_to_bohr(1.128), "6-31G"), "hf_ccpvdz": (["F", "H"], mol.angstrom_to_bohr(0.917), "cc-pVDZ"),
           "ne_ccpvdz": (["NE"], None, "cc-pVDZ")}


@pytest.fixture(scope="module")
def mp3_golden(golden):
    z = golden("mp3_systems")
    out = {}
    for key in z.files:
        tag, name = key.split("__", 1)
        out.setdefault(tag, {})[name] = z[key]
    return out


def _system(tag):
    sym, R, basis = SYSTEMS[tag]
    atoms = mol.make_atoms(sym, R)
    shells = mol.build_shells(atoms, basis)
    return shells, mol.expand_cartesian_aos(shells)


def _synthetic(n_sph):
    counts = mol.synthetic_counts(n_sph)
    atoms = mol.make_atoms(["AR", "AR"], 7.1)
    shells = mol.build_shells(atoms, {18: mol.even_tempered_basis(*counts)})
    return atoms, shells, mol.expand_cartesian_aos(shells)


def _reset(engine):
    engine._check(engine._L.tf_set_eri_layout(engine._ctx, -1))


def _terms(r):
    return np.array([r["E_pp"], r["E_hh"], r["E_ring"]])


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(1e-300, np.abs(np.asarray(b)))


@pytest.fixture(scope="module")
def n2_tz():
    shells, aos = _system("n2_ccpvtz")
    return aos, mr.dense_eri(aos, shells)


@pytest.mark.parametrize("tag", list(SYSTEMS))
def test_reference_orbitals_against_goldens(engine, mp3_golden, tag):
    g = mp3_golden[tag]
    engine.set_basis(_system(tag)[1]).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed"
    nocc = int(g["n_occ"])
    for nf, pre in ((0, ""), (1, "fc1_"), (2, "fc2_")):
        r = engine.mp3_rhf(g["C"], g["eps"], nocc, nf)
        print(f"\n[{tag} fc{nf}] E_MP3 {r['E_MP3']:.12f} (golden {float(g[pre + 'E_MP3']):.12f}) pp {r['E_pp']:.3e} hh {r['E_hh']:.3e} "
              f"ring {r['E_ring']:.3e}")
        assert abs(r["E_MP3"] - float(g[pre + "E_MP3"])) < 1e-10
        assert abs(r["E_OS"] - float(g[pre + "E_OS"])) < 1e-10 and abs(r["E_SS"] - float(g[pre + "E_SS"])) < 1e-10
        m = engine.mp2_rhf(g["C"], g["eps"], nocc, nf)
        assert _rel(r["E_OS"], m["E_OS"]) < 1e-12 and _rel(r["E_SS"], m["E_SS"]) < 1e-12, (r, m)


def _random_orbitals(N, seed):
    rng = np.random.default_rng(seed)
    C = np.linalg.qr(rng.standard_normal((N, N)))[0]
    eps = np.concatenate([-np.linspace(20.0, 0.5, 24), np.linspace(0.3, 8.0, N - 24)])
    return C, eps


@pytest.mark.parametrize("width", [1, 7, 8, 12, 16, 20])
def test_widths_against_the_independent_checker(engine, n2_tz, width):
    """N2/cc-pVTZ, random orthonormal orbitals: one pair; 49 pairs (one partial batch of 64); 64 and 256 pairs (full batches only); 144
    and 400 pairs (several batches of 64, the last one partial)."""
    aos, E = n2_tz
    engine.set_basis(aos).build_eri(True)
    C, eps = _random_orbitals(engine.N, 30 + width)
    got = _terms(engine.mp3_rhf(C, eps, width))
    want = np.array(mr.restricted_terms(E, C, eps, width))
    print(f"\n[width {width}] rel err per term {_rel(got, want)}")
    assert np.all(_rel(got, want) < 1e-12), (width, got, want)


def test_layouts_agree(engine, mp3_golden, n2_tz):
    """packed (the ladder kernel) against rows and tiles (the exchange-build route) on N2/cc-pVTZ, and packed against tiles at synth-400."""
    g = mp3_golden["n2_ccpvtz"]
    try:
        e = {}
        for layout in ("packed", "rows", "tiles"):
            engine.set_basis(n2_tz[0]).build_eri(True, layout=layout)
            assert engine.eri_storage()["layout"] == layout
            e[layout] = _terms(engine.mp3_rhf(g["C"], g["eps"], 7, 1))
        for lt in ("rows", "tiles"):
            assert np.all(_rel(e[lt], e["packed"]) < 1e-12), (lt, e[lt], e["packed"])
        atoms, shells, aos = _synthetic(400)
        C, eps = _random_orbitals(400, 400)
        big = {}
        for layout in ("packed", "tiles"):
            engine.set_basis(aos).build_eri(True, layout=layout)
            assert engine.eri_storage()["layout"] == layout and engine.N == 400
            r = engine.mp3_rhf(C, eps, 18)
            big[layout] = _terms(r)
            print(f"\n[synth-400 {layout}] terms {big[layout]} seconds {r['seconds']}")
        assert np.all(_rel(big["tiles"], big["packed"]) < 1e-10), big
    finally:
        _reset(engine)
    engine.set_basis(n2_tz[0]).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed"


def test_repeatable_and_refusals(engine, mp3_golden):
    from tuna_amd.engine import Engine
    g = mp3_golden["n2_ccpvdz"]
    shells, aos = _system("n2_ccpvdz")
    engine.set_basis(aos).build_eri(True)
    a, b = engine.mp3_rhf(g["C"], g["eps"], 7), engine.mp3_rhf(g["C"], g["eps"], 7)
    assert all(a[k] == b[k] for k in ("E_pp", "E_hh", "E_ring", "E_OS", "E_SS"))
    L, ctx, N = engine._L, engine._ctx, engine.N
    C, eps = (np.ascontiguousarray(x, dtype=np.float64) for x in (g["C"], g["eps"]))
    e2, e3 = (np.ctypeslib.ctypes.c_double * 2)(), (np.ctypeslib.ctypes.c_double * 3)()
    p = lambda x: x.ctypes.data_as(np.ctypeslib.ctypes.c_void_p)   # noqa: E731
    bad = [(7, -1, p(C), p(eps), e2, e3), (7, 7, p(C), p(eps), e2, e3), (0, 0, p(C), p(eps), e2, e3), (N, 0, p(C), p(eps), e2, e3),
           (7, 0, None, p(eps), e2, e3), (7, 0, p(C), None, e2, e3), (7, 0, p(C), p(eps), None, e3), (7, 0, p(C), p(eps), e2, None)]
    for args in bad:
        assert L.tf_mp3_rhf(ctx, *args, None) == TF_EINVAL, args
    with Engine(0) as fresh:                                          # no tensor yet
        fresh.set_basis(aos)
        assert fresh._L.tf_mp3_rhf(fresh._ctx, 7, 0, p(C), p(eps), e2, e3, None) == TF_EINVAL
    with Engine(0, 0, 2) as half:                                     # rank 0 of two: sharding is not supported
        half.set_basis(aos).build_eri(True)
        assert half._L.tf_mp3_rhf(half._ctx, 7, 0, p(C), p(eps), e2, e3, None) == TF_EINVAL
    # the context stays usable
    r = engine.mp3_rhf(g["C"], g["eps"], 7)
    assert abs(r["E_MP3"] - float(g["E_MP3"])) < 1e-10
    # the ladder probe: its refusals, each followed by a call that works
    T = np.random.default_rng(5).standard_normal((2, N, N))
    Z, out = engine.mp3_ladder_probe(T), np.zeros_like(T)
    assert np.all(np.isfinite(Z)) and np.abs(Z).max() > 0
    for args in ((0, p(T), p(out)), (-1, p(T), p(out)), (2, None, p(out)), (2, p(T), None)):
        assert L.tf_mp3_ladder_probe(ctx, *args) == TF_EINVAL, args
        assert np.array_equal(engine.mp3_ladder_probe(T), Z)
    assert L.tf_mp3_ladder_probe(None, 2, p(T), p(out)) == TF_EINVAL
    with Engine(0) as fresh:                                          # no tensor yet
        fresh.set_basis(aos)
        assert fresh._L.tf_mp3_ladder_probe(fresh._ctx, 2, p(T), p(out)) == TF_EINVAL
        fresh.build_eri(True)
        assert np.array_equal(fresh.mp3_ladder_probe(T), Z)
    with Engine(0, 0, 2) as half:                                     # rank 0 of two
        half.set_basis(aos).build_eri(True)
        assert half._L.tf_mp3_ladder_probe(half._ctx, 2, p(T), p(out)) == TF_EINVAL
    try:
        for layout in ("rows", "tiles"):
            engine.set_basis(aos).build_eri(True, layout=layout)
            assert engine.eri_storage()["layout"] == layout
            assert L.tf_mp3_ladder_probe(ctx, 2, p(T), p(out)) == TF_EINVAL
            with pytest.raises(TunaError):
                engine.mp3_ladder_probe(T)
            r = engine.mp3_rhf(g["C"], g["eps"], 7)
            assert abs(r["E_MP3"] - float(g["E_MP3"])) < 1e-10
    finally:
        _reset(engine)
    engine.set_basis(aos).build_eri(True)
    assert engine.eri_storage()["layout"] == "packed" and np.array_equal(engine.mp3_ladder_probe(T), Z)
    assert not np.any(out)                                            # (no refused call wrote anything)


def test_input_lines(engine, mp3_golden):
    from tuna_amd.energy import run
    n2 = mp3_golden["n2_ccpvtz"]
    E_SCF, E_OS, E_SS, E3 = (float(n2[k]) for k in ("E_SCF", "E_OS", "E_SS", "E_MP3"))
    cases = [("SPE : N N 1.0977 : MP3 CC-PVTZ : EXTREME", E_SCF + E_OS + E_SS + E3),
             ("SPE : N N 1.0977 : SCS-MP3 CC-PVTZ : EXTREME", E_SCF + float(n2["scs_E_corr"])),
             ("SPE : N N 1.0977 : SCS-MP3 CC-PVTZ : EXTREME MP3S 0.3 SSS 0.5 OSS 1.1", E_SCF + 0.5 * E_SS + 1.1 * E_OS + 0.3 * E3)]
    text = []
    for line, want in cases:
        log = []
        out = run(line, silent=False, engine=engine, log=log.append)
        print(f"\n[{line}] E = {out.energy:.10f} (golden {want:.10f}, d {out.energy - want:.1e})")
        assert abs(out.energy - want) < 1e-8, (line, out.energy, want)
        assert out.correlation_energy_mp3 == out.mp3["E_MP3_scaled"]
        text += log
    text = "\n".join(text)
    for s in ("MP3 correlation energy:", "Scaling for MP3: 0.250", "Scaling for MP3: 0.300", "Scaled MP3 correlation energy:",
              "SCS-MP3 correlation energy:", "Correlation energy from MP3:", "Correlation energy from SCS-MP3:", "Total correlation energy:",
              "Same spin contribution:", "Opposite spin contribution:", "MP2 correlation energy:"):
        assert s in text, s
    for line in ("SPE : O O 1.2075 : MP3 STO-3G : ML 3", "SPE : N N 1.0977 : UMP3 STO-3G", "SPE : N N 1.0977 : MP3 STO-3G : DIPOLE"):
        with pytest.raises(TunaError):
            run(line, engine=engine)
