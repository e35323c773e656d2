"""GPU: the matrix-core kernel of the exchange-correlation kernel build and its slab sum on their own (tf_xc_kernel_probe: the very
routine tf_xc_kernel_rhf and tf_tddft_rhf call, tuna_amd/csrc/tf_xckernel.hip.h) against np.einsum in float64, element by element,
on random orbital values and weights of both signs.  The shapes (o, v, G) walk every path of the kernel: one element and one
grid point; fewer points than a k-step of four and than a chunk; v < 16 (a 16-row strip spans several i) and v > 16; dim = 34 and 77
(one partial tile), 65 (one element past a tile: a diagonal tile, an off-diagonal tile of one column and a diagonal tile of one
element), 200 (four row blocks, ten tiles); G = 1030 and 4099 (several slabs with a ragged last chunk) and G = 2 slab + 3 (the last
slab starts three points before the end).

The bound.  An element is a sum of G terms u psi psi psi psi.  The kernel rounds the two pair products and the scaled right operand
(three roundings per term) and adds the terms with fused multiply-adds (one rounding per addition); the einsum rounds as many products
and additions in some other order.  Either result therefore differs from the exact sum by at most gamma_(G + 3) S in units of the unit
roundoff eps / 2, S = sum_g |u psi psi psi psi| -- whatever the order of the additions -- and the two from each other by twice that,
which 2 gamma_G S with gamma_G = G eps / (1 - G eps) and eps = 2^-52 covers for every G >= 3 and equals four roundings per side at
G = 1.  Nothing in it is fitted to what the kernel returns."""
import numpy as np
import pytest

from tuna_amd._lib import TunaError
from tuna_amd.engine import Engine

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SLAB = Engine.xc_kernel_plan(1, 1)["slab_min"]
SHAPES = [(1, 1, 1), (1, 1, 5), (3, 5, 7), (2, 17, 1030), (7, 11, 4099), (5, 40, 2 * SLAB + 3), (5, 13, 300)]


def operands(o, v, G, seed=0):
    rng = np.random.default_rng(1000 * o + 10 * v + G + seed)
    return rng.standard_normal((o, G)), rng.standard_normal((v, G)), rng.standard_normal(G), rng.standard_normal(G)


def reference(po, pv, u):
    """(K, S): the einsum and the sum of the magnitudes of its terms"""
    T = (po[:, None, :] * pv[None, :, :]).reshape(-1, po.shape[1])
    return np.einsum("pg,g,qg->pq", T, u, T), np.einsum("pg,g,qg->pq", np.abs(T), np.abs(u), np.abs(T))


@pytest.mark.parametrize("o,v,G", SHAPES)
def test_probe_against_einsum(engine, o, v, G):
    po, pv, us, ut = operands(o, v, G)
    KS, KT = engine.xc_kernel_probe(po, pv, us, ut)
    plan = Engine.xc_kernel_plan(o * v, G)
    gamma = G * EPS / (1 - G * EPS)
    worst = 0.0
    for K, u in ((KS, us), (KT, ut)):
        want, S = reference(po, pv, u)
        assert K.shape == want.shape and np.isfinite(K).all()
        ratio = (np.abs(K - want) / (2 * gamma * S)).max()
        worst = max(worst, ratio)
        assert np.array_equal(K, K.T)
    print(f"\n[o {o} v {v} G {G}] dim {o * v} tiles {plan['n_tiles']} slabs {plan['n_slabs']} x {plan['slab_len']} max |d| / (2 gamma_G S) = {worst:.3f}")
    assert worst <= 1.0
    again = engine.xc_kernel_probe(po, pv, us, ut)
    assert np.array_equal(again[0], KS) and np.array_equal(again[1], KT)


def test_equal_weights_give_equal_matrices(engine):
    """u_T = u_S: the two accumulator sets run the same operations on the same values"""
    po, pv, us, _ = operands(5, 40, 2 * SLAB + 3, seed=7)
    KS, KT = engine.xc_kernel_probe(po, pv, us, us)
    assert np.array_equal(KS, KT) and np.array_equal(KS, KS.T)


def test_shapes_exercise_the_plan():
    """what the docstring says of the shapes, from the plan itself"""
    plans = {s: Engine.xc_kernel_plan(s[0] * s[1], s[2]) for s in SHAPES}
    assert plans[(5, 13, 300)]["n_b"] == 2 and 5 * 13 == plans[(5, 13, 300)]["tile"] + 1
    assert plans[(5, 40, 2 * SLAB + 3)]["n_tiles"] == 10
    p = plans[(5, 40, 2 * SLAB + 3)]
    assert p["n_slabs"] >= 2 and (p["n_slabs"] - 1) * p["slab_len"] < 2 * SLAB + 3 <= p["n_slabs"] * p["slab_len"]
    assert plans[(7, 11, 4099)]["n_slabs"] > 2 and 4099 % plans[(7, 11, 4099)]["chunk"] != 0
    assert plans[(2, 17, 1030)]["n_slabs"] > 1


def test_probe_refusals(engine):
    po, pv, us, ut = operands(2, 3, 9)
    first = engine.xc_kernel_probe(po, pv, us, ut)
    L, ctx = engine._L, engine._ctx
    from tuna_amd._lib import ptr
    K = np.zeros((6, 6))
    bad = [(0, 3, 9, ptr(po), ptr(pv), ptr(us), ptr(ut), ptr(K), ptr(K)), (2, 0, 9, ptr(po), ptr(pv), ptr(us), ptr(ut), ptr(K), ptr(K)),
           (2, 3, 0, ptr(po), ptr(pv), ptr(us), ptr(ut), ptr(K), ptr(K)), (2, 3, 9, None, ptr(pv), ptr(us), ptr(ut), ptr(K), ptr(K)),
           (2, 3, 9, ptr(po), ptr(pv), None, ptr(ut), ptr(K), ptr(K)), (2, 3, 9, ptr(po), ptr(pv), ptr(us), ptr(ut), ptr(K), None)]
    for args in bad:
        assert L.tf_xc_kernel_probe(ctx, *args) == -1, args
        assert "tf_xc_kernel_probe" in L.tf_last_error(ctx).decode()
    again = engine.xc_kernel_probe(po, pv, us, ut)                      # the context stays usable
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
    with pytest.raises(ValueError):
        engine.xc_kernel_probe(po, pv[:, :5], us, ut)
    with pytest.raises(TunaError):
        Engine.xc_kernel_plan(0, 5)
