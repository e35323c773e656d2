"""CPU: the independent spin-orbital CIS(D) of tests/cisd_reference.py against every E_D of the reference program
(tests/golden/cisd_systems.npz), and the spin-adapted working equations the library evaluates (cisd_reference.working_equations, a NumPy
restatement with no three-virtual block) against the spin-orbital numbers part by part.

Measured here on the CPU, the largest over all 114 stored states (seven systems, frozen 0 and 1, CIS and for CO/6-31G TDHF):
|E_D spin-orbital - golden| = 2.9e-16 Eh, |E_D working equations - golden| = 3.1e-16 Eh; the parts of the working equations against
the spin-orbital parts 1.3e-15 (direct) and 1.5e-15 (indirect) relative to the sum of the magnitudes of the part's terms.  GOLDEN_TOL and
SPLIT_TOL are ten times the larger of each pair."""
import numpy as np
import pytest

import cisd_reference as cd
from test_cis_reference import SYSTEMS, split, system

GOLDEN_TOL = 3.1e-15              # Eh per state
SPLIT_TOL = 1.5e-14               # per part, relative to the sum of the magnitudes of its terms
MIN_DENOMINATOR = 0.1             # Eh: what tools/make_golden_cisd.py keeps
S_FLOOR = 1e-3                    # Eh, added to the scale of a part: the direct part of the H2/STO-3G triplet is exactly 0 (its only double
                                  # excitation is a singlet), and every other part of every stored state has a scale above 1e-2 Eh


@pytest.fixture(scope="module")
def goldens(golden):
    return split(golden("cis_systems")), split(golden("cisd_systems"))


def runs(gd):
    """(method, n_frozen) of the stored runs of one system"""
    return sorted({(k.split("_fc")[0], int(k.split("_fc")[1][0])) for k in gd if k.endswith("_E_D")})


def test_golden_file_holds_the_states(goldens):
    gc, gd = goldens
    assert set(gd) == set(SYSTEMS) == set(gc)
    for tag, d in gd.items():
        nocc, N = int(gc[tag]["n_occ"]), len(gc[tag]["eps"])
        want = [("CIS", nf) for nf in ((0, 1) if nocc > 1 else (0,))] + ([("TDHF", 0), ("TDHF", 1)] if tag == "co_631g" else [])
        assert runs(d) == sorted(want), tag
        for method, nf in runs(d):
            pre = f"{method}_fc{nf}_"
            o, v = nocc - nf, N - nocc
            n = len(d[pre + "E_D"])
            assert d[pre + "b"].shape == (n, o, v) and all(len(d[pre + k]) == n for k in ("omega", "triplet", "min_denominator", "index"))
            assert np.all(d[pre + "min_denominator"] > MIN_DENOMINATOR) and set(d[pre + "triplet"].tolist()) <= {0, 1}
            for flag in (0, 1):
                assert np.sum(d[pre + "triplet"] == flag) >= (3 if o * v >= 4 else 1), (tag, pre, flag)
            if method == "CIS":                                   # (TDHF: b = X + Y, whose norm is not 1)
                assert np.abs(np.sum(d[pre + "b"] ** 2, axis=(1, 2)) - 1).max() < 1e-12
            # the states are those of the CIS golden file
            assert np.abs(d[pre + "omega"] - gc[tag][pre + "energies"][d[pre + "index"]]).max() < 1e-13
            assert np.array_equal(d[pre + "triplet"], gc[tag][pre + "labels"][d[pre + "index"]])


@pytest.mark.parametrize("tag", list(SYSTEMS))
def test_both_forms_against_the_golden(goldens, tag):
    gc, gd = goldens
    g, d = gc[tag], gd[tag]
    shells, aos = system(tag)
    E = cd.dense_eri(aos, shells)
    C, eps, nocc = g["C"], g["eps"], int(g["n_occ"])
    for nf in sorted({nf for _, nf in runs(d)}):
        prep = cd.prepare(E, C, eps, nocc, nf)
        for method in [m for m, f in runs(d) if f == nf]:
            pre = f"{method}_fc{nf}_"
            worst = np.zeros(5)
            for b, w, flag, E_D, dmin in zip(d[pre + "b"], d[pre + "omega"], d[pre + "triplet"], d[pre + "E_D"], d[pre + "min_denominator"]):
                r = cd.correction(prep, b, float(w), int(flag))
                ed, ei = cd.working_equations(E, C, eps, nocc, nf, b, float(w), int(flag))
                worst = np.maximum(worst, [abs(r["E_D"] - E_D), abs(ed + ei - E_D), abs(ed - r["E_direct"]) / (r["S_direct"] + S_FLOOR),
                                           abs(ei - r["E_indirect"]) / (r["S_indirect"] + S_FLOOR), abs(r["min_denominator"] - dmin)])
            print(f"\n[{tag} {pre}] spin-orbital d {worst[0]:.1e} working equations d {worst[1]:.1e} direct {worst[2]:.1e} indirect {worst[3]:.1e} "
                  f"min denominator d {worst[4]:.1e}")
            assert worst[0] < GOLDEN_TOL and worst[1] < GOLDEN_TOL and worst[2] < SPLIT_TOL and worst[3] < SPLIT_TOL and worst[4] < 1e-13


def test_a_triplet_is_not_a_singlet(goldens):
    """the flag matters: the same vector as a singlet and as a triplet differs in both parts (CO/6-31G, the lowest stored state)"""
    gc, gd = goldens
    g, d = gc["co_631g"], gd["co_631g"]
    shells, aos = system("co_631g")
    prep = cd.prepare(cd.dense_eri(aos, shells), g["C"], g["eps"], int(g["n_occ"]), 0)
    b, w = d["CIS_fc0_b"][0], float(d["CIS_fc0_omega"][0])
    s, t = cd.correction(prep, b, w, 0), cd.correction(prep, b, w, 1)
    assert abs(s["E_direct"] - t["E_direct"]) > 1e-4 and abs(s["E_indirect"] - t["E_indirect"]) > 1e-4
