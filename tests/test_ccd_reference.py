"""CPU: the independent LCCD / CCD of tests/ccd_reference.py against the reference program's own iteration (tests/golden/ccd_systems.npz,
tools/make_golden_ccd.py) on the golden orbitals -- converged energy, the energy of every step and the step count, DIIS, NODIIS and
damping; its three forms against each other; LCCD's first step against MP2 + MP3.  tests/test_gpu_ccd.py then judges the library by it."""
import numpy as np
import pytest

import ccd_reference as cr
import mp3_reference as mr
from test_mp3_reference import SYSTEMS, _random_case, dense

GOLD_LOOP = dict(conv_delta_E=1e-11, amp_conv=1e-10, diis=True, max_diis=6)
METHODS = ("LCCD", "CCD")


def split(z):
    out = {}
    for key in z.files:
        tag, name = key.split("__", 1)
        out.setdefault(tag, {})[name] = z[key]
    return out


@pytest.fixture(scope="module")
def ccd_golden(golden):
    return split(golden("ccd_systems"))


@pytest.fixture(scope="module")
def mp3_golden(golden):
    return split(golden("mp3_systems"))


def test_golden_systems(ccd_golden):
    assert {"n2_ccpvdz", "n2_ccpvtz", "hf_ccpvdz", "ne_ccpvdz"} <= set(ccd_golden) <= set(SYSTEMS)


def check_against_golden(r, g, pre, what):
    want = g[pre + "energies"]
    print(f"\n[{what}] E_corr {r['energies'][-1]:.12f} (golden {float(g[pre + 'E_corr']):.12f}) steps {r['n_iter']} (golden {int(g[pre + 'n_iter'])}) "
          f"max step diff {np.abs(np.array(r['energies'])[:len(want)] - want[:r['n_iter']]).max():.1e}")
    assert r["converged"] and r["n_iter"] == int(g[pre + "n_iter"]), what
    assert abs(r["energies"][-1] - float(g[pre + "E_corr"])) < 1e-9, what
    assert np.abs(np.array(r["energies"]) - want).max() < 1e-8, what
    assert abs(r["E_MP2"] - float(g[pre + "E_MP2"])) < 1e-10, what


@pytest.mark.parametrize("tag", ["n2_ccpvdz", "co_631g", "hf_ccpvdz", "ne_ccpvdz"])
def test_restricted_checker_reproduces_the_goldens(ccd_golden, mp3_golden, tag):
    g, m = ccd_golden[tag], mp3_golden[tag]
    E = dense(tag)
    for method in METHODS:
        for nf in (0, 1):
            r = cr.restricted_iterations(E, m["C"], m["eps"], int(m["n_occ"]), nf, method, 100, **GOLD_LOOP)
            check_against_golden(r, g, f"{method}_fc{nf}_", f"{tag} {method} fc{nf}")
            assert abs(r["E_MP2"] - float(m[("", "fc1_")[nf] + "E_OS"]) - float(m[("", "fc1_")[nf] + "E_SS"])) < 1e-10


def _blocks(E, C, eps, n_occ, n_frozen):
    Co, Cv, eo, ev = mr._windows(C, eps, n_occ, n_frozen)
    ovov, oovv, oooo = mr.mo_tensor(E, Co, Cv, Co, Cv), mr.mo_tensor(E, Co, Co, Cv, Cv), mr.mo_tensor(E, Co, Co, Co, Co)
    return ovov, oovv, oooo, (lambda T: np.einsum("mlns,pls->pmn", E, T, optimize=True)), Cv, eo, ev


def test_from_blocks_reproduces_the_goldens_of_n2_ccpvtz(ccd_golden, mp3_golden):
    """the largest system through the form that never makes (ac|bd)"""
    g, m = ccd_golden["n2_ccpvtz"], mp3_golden["n2_ccpvtz"]
    E = dense("n2_ccpvtz")
    for method in METHODS:
        r = cr.iterations_from_blocks(*_blocks(E, m["C"], m["eps"], 7, 1), method, 100, **GOLD_LOOP)
        check_against_golden(r, g, f"{method}_fc1_", f"n2_ccpvtz {method} fc1")


def test_nodiis_and_damping_reproduce_the_goldens(ccd_golden, mp3_golden):
    g, m = ccd_golden["n2_ccpvdz"], mp3_golden["n2_ccpvdz"]
    E = dense("n2_ccpvdz")
    for method in METHODS:
        plain = cr.restricted_iterations(E, m["C"], m["eps"], 7, 0, method, 100, **dict(GOLD_LOOP, diis=False))
        check_against_golden(plain, g, f"{method}_nodiis_", f"{method} NODIIS")
        damped = cr.restricted_iterations(E, m["C"], m["eps"], 7, 0, method, 100, damping=0.3, **GOLD_LOOP)
        check_against_golden(damped, g, f"{method}_damp03_", f"{method} CORRDAMP 0.3")
        assert plain["n_iter"] >= int(g[f"{method}_fc0_n_iter"])


def _small_cases(mp3_golden):
    for tag, nf in (("hf_ccpvdz", 0), ("ne_ccpvdz", 2)):
        g = mp3_golden[tag]
        yield f"{tag} fc{nf}", dense(tag), g["C"], g["eps"], int(g["n_occ"]), nf
    for N, n_occ, nf in ((9, 3, 0), (12, 5, 1)):
        E, C, eps = _random_case(N, n_occ, 300 + N)
        yield f"random {N}", 0.02 * E, C, eps, n_occ, nf          # (scaled: amplitudes well below 1)


@pytest.mark.parametrize("method", METHODS)
def test_spin_orbital_restricted_and_from_blocks_agree(mp3_golden, method):
    """one, two and three plain steps and four damped ones: the alpha-beta block of the spin-orbital amplitudes, the restricted amplitudes
    and the amplitudes from the blocks; five steps with DIIS and damping: restricted and from the blocks (a DIIS over all spin-orbital
    amplitudes weighs the error vectors differently: another extrapolation, not compared); t_ijab = t_jiba after every step."""
    for what, E, C, eps, n_occ, nf in _small_cases(mp3_golden):
        for k, loop in ((1, {}), (2, {}), (3, {}), (4, dict(damping=0.2)), (5, dict(diis=True, max_diis=3, damping=0.2))):
            rs = cr.restricted_iterations(E, C, eps, n_occ, nf, method, k, **loop)
            so = cr.spin_orbital_iterations(E, C, eps, n_occ, nf, method, k, **dict(loop, diis=False))
            fb = cr.iterations_from_blocks(*_blocks(E, C, eps, n_occ, nf), method, k, batch=5, **loop)
            scale = np.abs(rs["t"]).max()
            print(f"\n[{what} {method} k={k}] max|t| {scale:.3f} so-rs {np.abs(so['t'] - rs['t']).max() / scale:.1e} "
                  f"fb-rs {np.abs(fb['t'] - rs['t']).max() / scale:.1e}")
            assert scale < 1.0
            assert np.abs(fb["t"] - rs["t"]).max() <= 1e-12 * scale, (what, k)
            assert np.allclose(fb["energies"], rs["energies"], rtol=1e-12, atol=0)
            for r in (rs, fb):
                assert np.abs(r["t"] - r["t"].transpose(1, 0, 3, 2)).max() <= 1e-15 * scale
            if loop.get("diis"):
                continue
            assert np.abs(so["t"] - rs["t"]).max() <= 1e-12 * scale, (what, k)
            assert np.allclose(so["energies"], rs["energies"], rtol=1e-12, atol=0)
            # the same-spin block of the spin-orbital amplitudes is the antisymmetrised closed-shell t
            aa = so["t_so"][0::2, 0::2, 0::2, 0::2]
            assert np.abs(aa - (rs["t"] - rs["t"].transpose(0, 1, 3, 2))).max() <= 1e-12 * scale


def test_lccd_step_one_is_mp2_plus_mp3(mp3_golden):
    for tag in ("n2_sto3g", "hf_ccpvdz", "n2_ccpvdz"):
        g = mp3_golden[tag]
        E = dense(tag)
        for nf, pre in ((0, ""), (1, "fc1_")):
            r = cr.restricted_iterations(E, g["C"], g["eps"], int(g["n_occ"]), nf, "LCCD", 1)
            e2 = float(g[pre + "E_OS"]) + float(g[pre + "E_SS"])
            assert abs(r["E_MP2"] - e2) < 1e-10
            assert abs(r["energies"][0] - (e2 + float(g[pre + "E_MP3"]))) < 1e-10, (tag, nf)
            want = r["E_MP2"] + sum(mr.restricted_terms(E, g["C"], g["eps"], int(g["n_occ"]), nf))
            assert abs(r["energies"][0] - want) <= 1e-12 * abs(want), (tag, nf)
    E, C, eps = _random_case(11, 4, 5)
    r = cr.restricted_iterations(E, C, eps, 4, 1, "LCCD", 1)
    want = r["E_MP2"] + sum(mr.restricted_terms(E, C, eps, 4, 1))
    assert abs(r["energies"][0] - want) <= 1e-12 * abs(want)


def test_singular_diis_matrix_clears_the_history():
    """a step function that stops changing gives zero error vectors: B is singular, the loop carries on without extrapolating"""
    t0 = np.ones((1, 1, 2, 2))
    r = cr.iterate(lambda t: 0.5 * t0, lambda t: float(t.sum()), t0, 6, diis=True, max_diis=3)
    assert r["n_iter"] == 6 and np.array_equal(r["t"], 0.5 * t0)
