"""CPU: the independent LCCSD / QCISD / CCSD of tests/ccsd_reference.py against the reference program's own iteration
(tests/golden/ccsd_systems.npz, tools/make_golden_ccsd.py) on the golden orbitals -- converged energy, the energy of every step, the step
count, the final t1, DIIS, NODIIS and damping; its three forms against each other (the printed agreement is the noise floor under the
tolerances of tests/test_gpu_ccsd.py); the staging of the from-blocks form (one batch loop of the ladder callback per step, nothing with
three virtual indices).  tests/test_gpu_ccsd.py then judges the library by the dense closed-shell form."""
import numpy as np
import pytest

import ccsd_reference as sr
import mp3_reference as mr
from test_ccd_reference import split
from test_mp3_reference import SYSTEMS, _random_case, dense

GOLD_LOOP = dict(conv_delta_E=1e-11, amp_conv=1e-10, diis=True, max_diis=6)
METHODS = sr.METHODS


@pytest.fixture(scope="module")
def ccsd_golden(golden):
    return split(golden("ccsd_systems"))


@pytest.fixture(scope="module")
def mp3_golden(golden):
    return split(golden("mp3_systems"))


def test_golden_systems(ccsd_golden):
    assert {"n2_ccpvdz", "n2_ccpvtz", "hf_ccpvdz", "ne_ccpvdz"} <= set(ccsd_golden) <= set(SYSTEMS)
    for tag, g in ccsd_golden.items():
        for method in METHODS:
            for nf in (0, 1):
                pre = f"{method}_fc{nf}_"
                assert float(g[pre + "E_singles"]) == 0.0
                assert (float(g[pre + "E_disconnected"]) == 0.0) == (method != "CCSD")
                assert 0.006 < float(g[pre + "t1_norm"]) < 0.08


def check_against_golden(r, g, pre, what):
    want = g[pre + "energies"]
    print(f"\n[{what}] E_corr {r['energies'][-1]:.12f} (golden {float(g[pre + 'E_corr']):.12f}) steps {r['n_iter']} (golden {int(g[pre + 'n_iter'])}) "
          f"max step diff {np.abs(np.array(r['energies'])[:len(want)] - want[:r['n_iter']]).max():.1e} "
          f"max t1 diff {np.abs(r['t1'] - g[pre + 't1']).max():.1e}")
    assert r["converged"] and r["n_iter"] == int(g[pre + "n_iter"]), what
    assert abs(r["energies"][-1] - float(g[pre + "E_corr"])) < 1e-9, what
    assert np.abs(np.array(r["energies"]) - want).max() < 1e-8, what
    assert abs(r["E_MP2"] - float(g[pre + "E_MP2"])) < 1e-10, what
    assert np.abs(r["t1"] - g[pre + "t1"]).max() < 1e-8, what
    assert abs(r["E_connected"] - float(g[pre + "E_connected"])) < 1e-9 and abs(r["E_disconnected"] - float(g[pre + "E_disconnected"])) < 1e-9, what


@pytest.mark.parametrize("tag", ["n2_ccpvdz", "co_631g", "hf_ccpvdz", "ne_ccpvdz"])
def test_restricted_checker_reproduces_the_goldens(ccsd_golden, mp3_golden, tag):
    g, m = ccsd_golden[tag], mp3_golden[tag]
    E = dense(tag)
    for method in METHODS:
        for nf in (0, 1):
            r = sr.restricted_iterations(E, m["C"], m["eps"], int(m["n_occ"]), nf, method, 100, **GOLD_LOOP)
            check_against_golden(r, g, f"{method}_fc{nf}_", f"{tag} {method} fc{nf}")


def _blocks(E, C, eps, n_occ, n_frozen):
    Co, Cv, eo, ev = mr._windows(C, eps, n_occ, n_frozen)
    ovov, oovv = mr.mo_tensor(E, Co, Cv, Co, Cv), mr.mo_tensor(E, Co, Co, Cv, Cv)
    oooo, ooov = mr.mo_tensor(E, Co, Co, Co, Co), mr.mo_tensor(E, Co, Co, Co, Cv)

    def jk_of(Dm):
        return np.einsum("mnls,ls->mn", E, Dm, optimize=True), np.einsum("mlsn,ls->mn", E, Dm, optimize=True)
    return (ovov, oovv, oooo, ooov, (lambda T: np.einsum("mlns,pls->pmn", E, T, optimize=True)),
            (lambda C1, C2, C3, C4: mr.mo_tensor(E, C1, C2, C3, C4)), jk_of, Co, Cv, eo, ev)


def test_from_blocks_reproduces_the_goldens_of_n2_ccpvtz(ccsd_golden, mp3_golden):
    """the largest system through the form that never makes a block with three virtual indices"""
    g, m = ccsd_golden["n2_ccpvtz"], mp3_golden["n2_ccpvtz"]
    E = dense("n2_ccpvtz")
    for method in METHODS:
        r = sr.iterations_from_blocks(*_blocks(E, m["C"], m["eps"], 7, 1), method, 100, **GOLD_LOOP)
        check_against_golden(r, g, f"{method}_fc1_", f"n2_ccpvtz {method} fc1")


def test_nodiis_and_damping_reproduce_the_goldens(ccsd_golden, mp3_golden):
    g, m = ccsd_golden["n2_ccpvdz"], mp3_golden["n2_ccpvdz"]
    E = dense("n2_ccpvdz")
    for method in METHODS:
        plain = sr.restricted_iterations(E, m["C"], m["eps"], 7, 0, method, 100, **dict(GOLD_LOOP, diis=False))
        check_against_golden(plain, g, f"{method}_nodiis_", f"{method} NODIIS")
        damped = sr.restricted_iterations(E, m["C"], m["eps"], 7, 0, method, 100, damping=0.3, **GOLD_LOOP)
        check_against_golden(damped, g, f"{method}_damp03_", f"{method} CORRDAMP 0.3")
        assert plain["n_iter"] >= int(g[f"{method}_fc0_n_iter"])


def _cases(mp3_golden):
    g = mp3_golden["n2_ccpvdz"]
    for nf in (0, 1):
        yield f"n2_ccpvdz fc{nf}", dense("n2_ccpvdz"), g["C"], g["eps"], 7, nf, True
    for tag, nf in (("hf_ccpvdz", 0), ("ne_ccpvdz", 2)):
        g = mp3_golden[tag]
        yield f"{tag} fc{nf}", dense(tag), g["C"], g["eps"], int(g["n_occ"]), nf, True
    for N, n_occ, nf in ((9, 3, 0), (12, 5, 1)):
        E, C, eps = _random_case(N, n_occ, 300 + N)
        yield f"random {N}", 0.02 * E, C, eps, n_occ, nf, True       # (scaled: amplitudes well below 1)
    # random orthonormal orbitals on the integrals of N2 / cc-pVTZ (N = 60): the spin-orbital form would hold 106^4 values, so here the
    # dense closed-shell form and the from-blocks form
    rng = np.random.default_rng(60)
    Q, _ = np.linalg.qr(rng.standard_normal((60, 60)))
    eps = np.sort(np.concatenate([-1.5 + 0.1 * rng.random(5), 0.6 + 2.0 * rng.random(55)]))
    yield "n2_ccpvtz random orbitals", 0.25 * dense("n2_ccpvtz"), Q, eps, 5, 1, False


@pytest.mark.parametrize("method", METHODS)
def test_spin_orbital_restricted_and_from_blocks_agree(mp3_golden, method):
    """one, two and three plain steps and four damped ones: the closed-shell blocks of the spin-orbital amplitudes, the dense restricted
    amplitudes and the amplitudes from the blocks; five steps with DIIS and damping: restricted and from the blocks (a DIIS over all
    spin-orbital amplitudes weighs the error vectors differently: another extrapolation, not compared); t_ijab = t_jiba after every step;
    the from-blocks form runs one batch loop of Z_of per step."""
    worst = 0.0
    for what, E, C, eps, n_occ, nf, with_so in _cases(mp3_golden):
        for k, loop in ((1, {}), (2, {}), (3, {}), (4, dict(damping=0.2)), (5, dict(diis=True, max_diis=3, damping=0.2))):
            rs = sr.restricted_iterations(E, C, eps, n_occ, nf, method, k, **loop)
            counts = {}
            fb = sr.iterations_from_blocks(*_blocks(E, C, eps, n_occ, nf), method, k, batch=5, counts=counts, **loop)
            o = n_occ - nf
            assert counts["loops"] == k and counts["Z_of"] == k * -(-o * o // 5)
            assert counts["mo_of"] == (2 * k if method == "CCSD" else 0) and counts["jk_of"] == (k if method == "CCSD" else 0)
            s2, s1 = np.abs(rs["t2"]).max(), np.abs(rs["t1"]).max()
            d2, d1 = np.abs(fb["t2"] - rs["t2"]).max() / s2, np.abs(fb["t1"] - rs["t1"]).max() / s1
            line = f"\n[{what} {method} k={k}] max|t2| {s2:.3f} max|t1| {s1:.3f} fb-rs t2 {d2:.1e} t1 {d1:.1e}"
            assert s2 < 1.0 and s1 < 1.0
            assert 0.0 < s1
            assert d2 <= 1e-12 and d1 <= 1e-12, (what, k)
            assert np.allclose(fb["energies"], rs["energies"], rtol=1e-12, atol=0)
            worst = max(worst, d2, d1)
            for r in (rs, fb):
                assert np.abs(r["t2"] - r["t2"].transpose(1, 0, 3, 2)).max() <= 1e-15 * s2
            if loop.get("diis") or not with_so or (what.startswith("n2") and k > 2):
                print(line)
                continue
            so = sr.spin_orbital_iterations(E, C, eps, n_occ, nf, method, k, **dict(loop, diis=False))
            e2, e1 = np.abs(so["t2"] - rs["t2"]).max() / s2, np.abs(so["t1"] - rs["t1"]).max() / s1
            print(line + f" so-rs t2 {e2:.1e} t1 {e1:.1e}")
            assert e2 <= 1e-12 and e1 <= 1e-12, (what, k)
            assert np.allclose(so["energies"], rs["energies"], rtol=1e-12, atol=0)
            worst = max(worst, e2, e1)
            # the same-spin block of the spin-orbital doubles is the antisymmetrised closed-shell t2; the beta singles are the alpha ones
            aa = so["t2_so"][0::2, 0::2, 0::2, 0::2]
            assert np.abs(aa - (rs["t2"] - rs["t2"].transpose(0, 1, 3, 2))).max() <= 1e-12 * s2
            assert np.abs(so["t1_so"][1::2, 1::2] - rs["t1"]).max() <= 1e-12 * s1 and np.abs(so["t1_so"][0::2, 1::2]).max() == 0.0
    print(f"\n[{method}] largest relative disagreement between the forms: {worst:.1e}")


def test_first_step_sees_no_singles(mp3_golden):
    """t1 = 0 in: the doubles of step one are LCCD's (LCCSD) and CCD's (QCISD, CCSD); the singles of step one are not zero"""
    import ccd_reference as cr
    g = mp3_golden["hf_ccpvdz"]
    E = dense("hf_ccpvdz")
    for method, doubles in (("LCCSD", "LCCD"), ("QCISD", "CCD"), ("CCSD", "CCD")):
        r = sr.restricted_iterations(E, g["C"], g["eps"], int(g["n_occ"]), 1, method, 1)
        d = cr.restricted_iterations(E, g["C"], g["eps"], int(g["n_occ"]), 1, doubles, 1)
        assert np.abs(r["t2"] - d["t"]).max() <= 1e-13 * np.abs(d["t"]).max()
        assert np.abs(r["t1"]).max() > 1e-4
        # the energy of step one holds CCSD's disconnected part, made of the new t1
        assert abs(r["energies"][0] - r["E_disconnected"] - d["energies"][0]) <= 1e-12 * abs(d["energies"][0])
