"""CPU: the infrastructure of tests/test_gpu_eri_shapes.py checks itself -- the systems have the sizes the slab settings are worked out
for, the seam geometries land on both sides of every branch of the kernels' Boys function, and the oracle's Boys function agrees with
50-digit values (tests/golden/boys_seams.npz, written by tools/make_golden_boys_seams.py) at every seam."""
import math

import numpy as np
import pytest

import eri_shapes as es
from oracle import oracle as orc

# tag: (Cartesian AOs, spherical AOs, shells, shell pairs, Cartesian bra rows, largest pair)
SIZES = {"n2_ccpvdz": (30, 28, 12, 78, 507, 36), "c2_n2_ccpvtz": (70, 60, 20, 210, 2653, 100), "high_l": (84, 53, 9, 45, 4173, 441),
         "f_mix": (68, 56, 16, 136, 2541, 100), "one_s": (1, 1, 1, 1, 1, 1), "two_s": (2, 2, 2, 3, 3, 1), "one_p": (3, 3, 1, 1, 9, 9),
         "one_d": (6, 5, 1, 1, 36, 36), "deep_p": (3, 3, 1, 1, 9, 9)}


@pytest.mark.parametrize("tag", sorted(SIZES))
def test_systems_have_the_sizes_the_slab_settings_assume(tag):
    _, shells, aos = es.system(tag)
    n_cart, n_sph, n_shell, n_pair, rows, largest = SIZES[tag]
    assert (aos.n, sum(s.n_sph for s in shells), len(shells), es.n_bra_pairs(shells), es.total_rows(shells), es.largest_pair(shells)) == \
           (n_cart, n_sph, n_shell, n_pair, rows, largest)
    R = es.r_mid(shells)
    assert R == max(largest, math.ceil(rows / 4)) and R >= largest
    if tag in es.SLAB_TAGS:
        assert math.ceil(rows / R) >= 4                                     # a cut at R_mid gives at least four slabs
    for world in (1, 2):
        assert sum(es.n_bra_pairs(shells, r, world) for r in range(world)) == n_pair
        if world == 2:
            assert sum(es.rank_rows(shells, r, 2) for r in range(2)) == rows
    assert len(es.ao_classes(shells, True)) == n_sph and len(es.ao_classes(shells, False)) == n_cart


def test_uncontracted_and_contracted_systems():
    """f_mix: every shell one primitive and every pair sum <= 6 (the team kernels' TF_TEAM_LMAX); high_l: pair sums above it;
    c2_n2_ccpvtz: two shells on the same primitives (families); deep_p: 100 primitive pairs in its one pair"""
    shells = es.system("f_mix")[1]
    assert all(len(s.exps) == 1 for s in shells) and 2 * max(s.L for s in shells) <= 6
    assert 2 * max(s.L for s in es.system("high_l")[1]) > 6
    tz = es.system("c2_n2_ccpvtz")[1]
    assert any(a is not b and a.atom == b.atom and a.L == b.L and len(a.exps) > 1 and np.array_equal(a.exps, b.exps) for a in tz for b in tz)
    assert len(es.system("deep_p")[1][0].exps) ** 2 * 2 * 12 * 2 > 3072        # both pairs' Hermite tables against eri_class_kernel's EB


def test_seam_system_and_distances():
    _, shells, aos = es.seam_system(6.0)
    assert aos.n == 114 and [s.L for s in shells] == [0, 1, 2, 3, 4, 5, 0] * 2
    assert all(len(s.exps) == 1 for s in shells) and [float(s.exps[0]) for s in shells[:7]] == [1.0] * 6 + [0.5]
    assert shells[7].origin[2] == 6.0 and shells[0].origin[2] == 0.0
    Rs = es.seam_distances()
    assert len(Rs) == 22 and len(set(Rs)) == 22 and min(Rs) > 0.0
    assert es.system(es.seam_tag(Rs[0]))[1][7].origin[2] == Rs[0]           # the tag keeps every bit of R


def test_seam_distances_land_on_both_sides_of_every_branch():
    """T = alpha * PQ * PQ in float64 as the kernels form it, for the probe quartets of every R"""
    Ts = sorted({T for R in es.seam_distances() for T in es.probe_T(R).values()})
    branches = [es.boys_branch(T) for T in Ts]
    for seam in es.SEAMS:
        i = int(seam / es.BOYS_STEP)                                        # the seam lies between grid rows i and i + 1
        near = [es.boys_branch(T)[1] for T in Ts if abs(T - seam) <= 4 * np.spacing(seam)]
        assert i in near and i + 1 in near, (seam, near)
    last = [T for T, b in zip(Ts, branches) if b == ("grid", 288)]
    assert last and max(last) == np.nextafter(36.0, 0.0) and min(last) <= 35.9375 + 4 * np.spacing(36.0)
    assert ("asymptotic", None) in branches and 36.0 in Ts                   # the first value of the asymptotic branch itself
    assert any(es.probe_T(R)["(AA|AB)"] == 36.0 for R in es.seam_distances())
    assert all(es.probe_T(R)["(AB|AB)"] == 0.0 and R != 0.0 for R in es.seam_distances())      # T == 0.0 in a two-centre system
    assert ("grid", 0) in branches and any(0.0 < T < 1e-15 for T in Ts)
    assert max(Ts) == 40000.0


def test_oracle_boys_function_at_the_seams(golden):
    """orc.boys against 50-digit values within 1e-14 relative, the bound tests/test_oracle.py uses below T = 50"""
    g = golden("boys_seams")
    T, F = g["T"], g["F"]
    assert F.shape == (len(T), 21) and T[0] == 0.0 and np.all(F > 0.0)
    for seam in es.SEAMS + (36.0, 45.0, 50.0, 65.0):
        assert {float(np.nextafter(seam, -np.inf)), seam, float(np.nextafter(seam, np.inf))} <= set(T.tolist())
    np.testing.assert_array_equal(F[0], 1.0 / (2.0 * np.arange(21) + 1.0))
    worst = (-1.0, 0.0, 0)
    for i, t in enumerate(T):
        for m in range(21):
            worst = max(worst, (abs(orc.boys(m, float(t)) - F[i, m]) / F[i, m], float(t), m))
    print(f"\n[eri-shapes] orc.boys against the 50-digit values: worst relative deviation {worst[0]:.3e} at T = {worst[1]!r}, m = {worst[2]}")
    assert worst[0] <= 1e-14, worst
