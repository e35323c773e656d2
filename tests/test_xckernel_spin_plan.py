"""CPU: the launch plan of the spin-blocked exchange-correlation kernel build (xck_spin_plan, xck_spin_block and xck_spin_tiles of
tuna_amd/csrc/tf_xckernel_plan.h, compiled with g++ through tests/xckernel_spin_model): blocks of 64 are cut per spin, so every tile
-- 64 x 64, or 64 x 128 from two adjacent column blocks of one spin -- has one pair of spins; every element p <= q of the compound
index lies in exactly one tile and the beta-alpha rectangle in none; an empty spin block has no block; the slabs tile [0, G) by the restricted plan's rule on this tile count; the sizes are what the host
allocates (the library's own export); and the plan is a pure function of (d_alpha, d_beta, G)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_xckernel_plan as rp

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
KEYS = ("n_b_alpha", "n_b_beta", "n_tiles", "n_slabs", "slab_len", "lds_bytes", "partial_doubles", "dim", "chunk", "slab_min", "tile", "row", "lds_limit", "cols")
D = [0, 1, 63, 64, 65, 129]
GRIDS = [1, 31, 32, 33, 255, 256, 257, 100000]


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(HERE, "xckernel_spin_model", "_build", "libxckernelspinplan.so")
        src = [os.path.join(HERE, "xckernel_spin_model", "xckernel_spin_plan.cpp"), os.path.join(HERE, "..", "tuna_amd", "csrc", "tf_xckernel_plan.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
            subprocess.check_call(["sh", os.path.join(HERE, "xckernel_spin_model", "build.sh")])
        L = C.CDLL(so)
        L.xcksm_plan.argtypes = [C.c_longlong, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p]
        L.xcksm_blocks.argtypes = [C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p]
        L.xcksm_tiles.argtypes = [C.c_longlong, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p]
        _LIB = L
    return _LIB


def plan(da, db, G, cols=0):
    """cols = 0: the library's default shape"""
    out = np.zeros(len(KEYS), dtype=np.int64)
    lib().xcksm_plan(da, db, G, cols, out.ctypes.data)
    return dict(zip(KEYS, (int(x) for x in out)))


def blocks(da, db, G):
    p = plan(da, db, G)
    b = np.zeros(3 * (p["n_b_alpha"] + p["n_b_beta"]), dtype=np.int64)
    lib().xcksm_blocks(da, db, G, b.ctypes.data)
    return b.reshape(-1, 3)


def tiles(da, db, G, cols):
    t = np.zeros(3 * plan(da, db, G, cols)["n_tiles"], dtype=np.int64)
    lib().xcksm_tiles(da, db, G, cols, t.ctypes.data)
    return t.reshape(-1, 3)


PAIRS = [(a, b) for a in D for b in D if a + b > 0]


@pytest.mark.parametrize("cols", [1, 2])
@pytest.mark.parametrize("da,db", PAIRS)
def test_every_element_lies_in_exactly_one_spin_pure_tile(da, db, cols):
    """The kernel's own arithmetic, replayed for both tile shapes: tile -> (row block, first column block, column blocks) from the list
    the host uploads (xck_spin_tiles), block -> (spin, first, offset) by xck_spin_block, the tile's rows and columns clipped to the
    spin's d, elements with column < row dropped.  Every p <= q is written once, nothing with q < p, a tile's rows all have one spin and
    its columns all have one spin, and no tile is without an element."""
    p, blk, til = plan(da, db, 257, cols), blocks(da, db, 257), tiles(da, db, 257, cols)
    T, dim, d = p["tile"], da + db, (da, db)
    assert p["dim"] == dim and p["n_b_alpha"] == -(-da // T) and p["n_b_beta"] == -(-db // T) and p["cols"] == cols
    nb = p["n_b_alpha"] + p["n_b_beta"]
    assert len(til) == p["n_tiles"] and len({tuple(t) for t in til}) == len(til)
    assert np.all(np.diff(til[:, 0]) >= 0)                                                       # row block by row block
    if cols == 1:
        assert [tuple(t[:2]) for t in til] == [(i, j) for i in range(nb) for j in range(i, nb)] and np.all(til[:, 2] == 1)
        assert p["n_tiles"] == nb * (nb + 1) // 2
    count = np.zeros((dim, dim), dtype=int)
    spin_of = np.array([0] * da + [1] * db)
    for bi, bj, nc in til:
        assert 1 <= nc <= cols
        (si, p0, offL), (sj, q0, offR) = blk[bi], blk[bj]
        assert all(blk[bj + c][0] == sj for c in range(nc))                                      # the column blocks of a tile have one spin
        assert si <= sj and offL == (da if si else 0) and offR == (da if sj else 0) and p0 % T == 0 and q0 % T == 0
        rows = offL + np.arange(p0, min(p0 + T, d[si]))
        cols_ = offR + np.arange(q0, min(q0 + nc * T, d[sj]))
        assert np.all(spin_of[rows] == si) and np.all(spin_of[cols_] == sj)                    # spin-pure: one weight vector
        rr, cc = np.meshgrid(rows, cols_, indexing="ij")
        keep = cc >= rr
        assert keep.any()                                                                        # no tile without an element
        np.add.at(count, (rr[keep], cc[keep]), 1)
    assert np.array_equal(count, np.triu(np.ones((dim, dim), dtype=int)))
    if da == 0 or db == 0:                                                                       # an empty spin block has no block and no tile
        assert (p["n_b_alpha"] == 0) == (da == 0) and (p["n_b_beta"] == 0) == (db == 0)
        assert np.all(blk[:, 0] == (1 if da == 0 else 0))


@pytest.mark.parametrize("cols", [1, 2])
@pytest.mark.parametrize("G", GRIDS)
@pytest.mark.parametrize("da,db", PAIRS)
def test_slabs_tile_the_grid_by_the_restricted_rule(da, db, G, cols):
    """slab s = [s slab_len, min(G, (s + 1) slab_len)): consecutive, none empty, whole chunks; and the cut is the restricted plan's for the
    same number of tiles (one function, xck_slab_cut, serves both plans)"""
    p = plan(da, db, G, cols)
    n, L = p["n_slabs"], p["slab_len"]
    assert n >= 1 and L % p["chunk"] == 0 and (n - 1) * L < G <= n * L and n <= 65535
    assert n == 1 or L >= p["slab_min"]
    same = [r for r in (rp.plan(k * p["tile"], G) for k in range(1, 12)) if r["n_tiles"] == p["n_tiles"]]
    for r in same:                                             # a restricted index with as many tiles
        assert (r["n_slabs"], r["slab_len"]) == (n, L)
    assert same or cols == 2


@pytest.mark.parametrize("da,db", PAIRS)
def test_sizes_match_what_the_host_allocates(da, db):
    from tuna_amd.engine import Engine
    for G in GRIDS:
        p, e = plan(da, db, G), Engine.xc_kernel_spin_plan(da, db, G)                          # the default shape on both sides
        assert all(p[k] == e[k] for k in ("n_b_alpha", "n_b_beta", "n_tiles", "n_slabs", "slab_len", "lds_bytes", "partial_doubles"))
        assert e["tile_cols"] == p["tile"] * p["cols"]
        for cols in (1, 2):
            p = plan(da, db, G, cols)
            assert p["partial_doubles"] == p["n_slabs"] * (da + db) ** 2
            # the kernel's static arrays: left operand [chunk][row], right operand [chunk][64 cols + 16] and ONE weight vector [chunk], doubles
            assert p["lds_bytes"] == 8 * (p["chunk"] * p["row"] + p["chunk"] * (cols * p["tile"] + 16) + p["chunk"]) <= 64 * 1024 <= p["lds_limit"]
            assert (cols * p["tile"] + 16) % 32 == 16 and p["n_slabs"] * p["n_tiles"] < 1024 + p["n_tiles"]


def test_plan_is_a_function_of_its_arguments_alone():
    first = [plan(a, b, G, c) for a, b in PAIRS for G in GRIDS for c in (1, 2)]
    assert [plan(a, b, G, c) for a, b in PAIRS for G in GRIDS for c in (1, 2)] == first
    src = open(os.path.join(HERE, "..", "tuna_amd", "csrc", "tf_xckernel_plan.h")).read()
    assert "#include <hip" not in src and "hipDeviceProp" not in src and "multiProcessorCount" not in src and "getenv" not in src
    assert plan(63, 65, 1000, 1) != plan(65, 63, 1000, 1) and plan(128, 0, 1000, 1)["n_tiles"] == 3 and plan(64, 64, 1000, 1)["n_tiles"] == 3
    assert plan(65, 63, 1000, 1)["n_tiles"] == 6             # 2 + 1 blocks: the last alpha block is padded, not continued into beta
    assert plan(65, 63, 1000, 2)["n_tiles"] == 5             # rows 0 and 1 (alpha): [a0 a1], [b0] each; row 2 (beta): [b0]
    assert plan(129, 0, 1000, 2)["n_tiles"] == 5             # three alpha blocks: groups [0 1], [2]; rows 0, 1 take both, row 2 the last
