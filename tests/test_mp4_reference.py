"""CPU: the independent MP4(SDQ) of tests/mp4_reference.py against the reference program's own run_restricted_MP4
(tests/golden/mp4_systems.npz, tools/make_golden_mp4.py) on the golden orbitals, all-electron and with one frozen orbital, SDQ and DQ;
its forms against each other on random data.  tests/test_gpu_mp4.py then judges the library by it."""
import numpy as np
import pytest

import mp3_reference as mr
import mp4_reference as m4
from test_ccd_reference import split
from test_mp3_reference import SYSTEMS, _random_case, dense

PARTS = ("E_S", "E_D", "E_Q", "E_MP4")


@pytest.fixture(scope="module")
def mp4_golden(golden):
    return split(golden("mp4_systems"))


@pytest.fixture(scope="module")
def mp3_golden(golden):
    return split(golden("mp3_systems"))


def test_golden_systems(mp4_golden, mp3_golden):
    assert set(mp4_golden) == set(mp3_golden) == set(SYSTEMS)
    for tag, g in mp4_golden.items():
        for nf in (0, 1):
            assert float(g[f"DQ_fc{nf}_E_S"]) == 0.0
            for k in ("E_D", "E_Q"):
                assert float(g[f"DQ_fc{nf}_{k}"]) == float(g[f"SDQ_fc{nf}_{k}"])
            assert abs(float(g[f"fc{nf}_E_MP3"]) - float(mp3_golden[tag][("", "fc1_")[nf] + "E_MP3"])) < 1e-12


@pytest.mark.parametrize("tag", list(SYSTEMS))
def test_checker_reproduces_the_goldens(mp4_golden, mp3_golden, tag):
    g, m = mp4_golden[tag], mp3_golden[tag]
    E = dense(tag)
    form = "restricted" if tag == "n2_ccpvtz" else "spin_orbital"       # (<ab||cd> of 106 spin orbitals: 1 GB)
    for nf in (0, 1):
        for level in ("SDQ", "DQ"):
            r = m4.components(E, m["C"], m["eps"], int(m["n_occ"]), nf, level, form=form)
            diffs = {k: r[k] - float(g[f"{level}_fc{nf}_{k}"]) for k in PARTS}
            print(f"\n[{tag} fc{nf} {level}] " + " ".join(f"d{k} {d:.1e}" for k, d in diffs.items()))
            for k, d in diffs.items():
                assert abs(d) < 1e-10, (tag, nf, level, k, d)
            assert abs(r["E_MP3"] - float(g[f"fc{nf}_E_MP3"])) < 1e-10
        assert m4.components(E, m["C"], m["eps"], int(m["n_occ"]), nf, "DQ", form=form)["E_S"] == 0.0


def _blocks(E, C, eps, n_occ, n_frozen):
    Co, Cv, eo, ev = mr._windows(C, eps, n_occ, n_frozen)
    return (mr.mo_tensor(E, Co, Cv, Co, Cv), mr.mo_tensor(E, Co, Co, Co, Cv),
            (lambda T: np.einsum("ilkj,pkl->pij", E, T.transpose(0, 2, 1), optimize=True)), Co, Cv, eo, ev)


@pytest.mark.parametrize("N, n_occ, n_frozen", [(9, 3, 0), (12, 5, 1), (10, 1, 0), (11, 4, 3)])
def test_forms_agree_on_random_data(N, n_occ, n_frozen):
    """spin-orbital and restricted steps; the singles as driven doubles, as the Hermitian form, and from the blocks (Z as the exchange
    matrix of the transposed argument, the way tests/test_gpu_mp4_large.py makes it)"""
    E, C, eps = _random_case(N, n_occ, 400 + N)
    E = 0.02 * E
    so = m4.components(E, C, eps, n_occ, n_frozen, form="spin_orbital")
    rs = m4.components(E, C, eps, n_occ, n_frozen, form="restricted")
    scale = abs(so["E_MP2"])
    for k in PARTS:
        assert abs(so[k] - rs[k]) <= 1e-12 * scale, (k, so[k], rs[k])
    herm = m4.singles_hermitian(E, C, eps, n_occ, n_frozen)
    fb, S = m4.singles_from_blocks(*_blocks(E, C, eps, n_occ, n_frozen), batch=4)
    assert abs(herm - so["E_S"]) <= 1e-12 * abs(so["E_S"])
    assert abs(fb - so["E_S"]) <= 1e-12 * S and S >= abs(so["E_S"]) * (1 - 1e-12)


@pytest.mark.parametrize("tag", ["n2_sto3g", "hf_ccpvdz", "n2_ccpvdz"])
def test_singles_from_blocks_reproduce_the_goldens(mp4_golden, mp3_golden, tag):
    g, m = mp4_golden[tag], mp3_golden[tag]
    E = dense(tag)
    for nf in (0, 1):
        fb, S = m4.singles_from_blocks(*_blocks(E, m["C"], m["eps"], int(m["n_occ"]), nf))
        assert abs(fb - float(g[f"SDQ_fc{nf}_E_S"])) < 1e-10, (tag, nf)
        assert S < 10 * abs(fb)


def test_unknown_level_or_form():
    E, C, eps = _random_case(6, 2, 1)
    with pytest.raises(ValueError):
        m4.components(E, C, eps, 2, 0, level="SDTQ")
    with pytest.raises(KeyError):
        m4.components(E, C, eps, 2, 0, form="other")
