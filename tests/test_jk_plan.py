"""CPU: the buffer plan of the packed Fock build (tuna_amd/csrc/tf_jk_plan.h, compiled with g++ through tests/packed_model) against
its formulas written out here in NumPy integers, on the inputs the library's own host tables give (tests/packed_tables.py): the shapes
two_s, one_p, c0_65, mid_17_9 of tests/fock_reference.py and N2/cc-pVTZ; one rank, rank 0 of two (every other shell pair; walks cut in
2 parts) and a rank of four that owns no row (4 parts); both pass types (ND = 1, 2), general and class-diagonal buffers.  Every size
and offset equals its formula; the regions of the two pass types are disjoint and inside their buffer; every extent is at least one double; in the
class-diagonal ypart buffer the ND = 2 region starts where the ND = 1 region ends."""
import numpy as np
import pytest

import fock_reference as fr
import packed_tables as pt
from tuna_amd import molecule as mol

TAGS = ("two_s", "one_p", "c0_65", "mid_17_9", "n2_ccpvtz")
RANKS = {"one rank": (None, 1), "rank 0 of 2": (0, 2), "rank without rows": ("none", 4)}
_INPUTS = {}


def shells_of(tag):
    if tag == "n2_ccpvtz":
        return mol.build_shells(mol.make_atoms(["N", "N"], mol.angstrom_to_bohr(1.0977)), "cc-pVTZ")
    return fr.system(tag)[1]


def inputs(tag, rank):
    """what jk_alloc_state hands to jk_plan, from the library's host tables of this shape and rank (built once per case)"""
    if (tag, rank) not in _INPUTS:
        shells = shells_of(tag)
        cls, dims = fr.ao_classes(shells), [s.n_sph for s in shells]
        who, world = RANKS[rank]
        npairs = len(dims) * (len(dims) + 1) // 2
        mine = None if who is None else (np.zeros(0, np.int32) if who == "none" else np.arange(npairs)[np.arange(npairs) % 2 == who])
        T = [pt.Tables(cls, dims, mine, world, pt.const(rb)) for rb in ("RB1", "RB2")]
        _INPUTS[(tag, rank)] = dict(N=T[0].N, n_rows=len(T[0].row_ij), NW=T[0].NW, MP=T[0].MP, RS=T[0].RS, NPtot=T[0].NPtot,
                                    n_groups=[len(t.groups) for t in T], ypart_len=[t.ypart_len for t in T], nseg=[t.nseg for t in T])
    return _INPUTS[(tag, rank)]


@pytest.mark.parametrize("rank", list(RANKS))
@pytest.mark.parametrize("tag", TAGS)
def test_sizes_equal_the_formulas(tag, rank):
    a = inputs(tag, rank)
    if rank == "rank without rows":
        assert a["n_rows"] == 0 and a["n_groups"] == [0, 0]
    else:
        assert a["n_rows"] > 0 and 1 <= a["MP"] <= RANKS[rank][1]
        assert a["MP"] == RANKS[rank][1] or tag in ("two_s", "one_p")       # (cut walks are covered: only the tiniest shapes have nothing to cut)
    P = pt.jk_plan(**a)
    N, NW, MP, RS, NPtot = (a[k] for k in ("N", "NW", "MP", "RS", "NPtot"))
    nrows, ng, y = max(1, a["n_rows"]), [max(1, g) for g in a["n_groups"]], a["ypart_len"]
    per_g = N * MP + RS
    want = {"Jrow": 2 * max(1, NW * MP) * nrows, "ypart": max(1, max(y[0], 2 * y[1])), "DI": (ng[0] + 2 * ng[1]) * per_g, "DJ": 3 * nrows * per_g,
            "Jt": 2 * max(a["nseg"]) * NPtot, "cd_ypart": max(1, y[0] + 2 * y[1])}
    want.update(cd_Jrow=want["Jrow"], cd_DI=want["DI"], cd_DJ=want["DJ"])
    assert {k: P[k] for k in pt.PLAN_SIZES} == want
    assert all(P[k] >= 1 for k in pt.PLAN_SIZES)


@pytest.mark.parametrize("nd", [1, 2])
@pytest.mark.parametrize("rank", list(RANKS))
@pytest.mark.parametrize("tag", TAGS)
def test_pass_offsets_and_strides_equal_the_formulas(tag, rank, nd):
    a = inputs(tag, rank)
    P = pt.jk_plan(**a)
    q = P["pass"][nd]
    N, NW, MP, RS, NPtot = (a[k] for k in ("N", "NW", "MP", "RS", "NPtot"))
    nrows, ng0, ng = max(1, a["n_rows"]), max(1, a["n_groups"][0]), max(1, a["n_groups"][nd - 1])
    per_g = N * MP + RS
    want = {"DI0": ng0 * per_g if nd == 2 else 0, "DJ0": nrows * per_g if nd == 2 else 0, "y0": 0, "y0_cd": max(0, a["ypart_len"][0]) if nd == 2 else 0,
            "DIr": nd * MP * ng * N, "DJr": nd * MP * nrows * N, "sP": N * N, "sPp": NPtot, "sy": a["ypart_len"][nd - 1], "sJd": MP * nrows * NW,
            "sDIc": MP * ng * N, "sDIr": ng * RS, "sDJc": MP * nrows * N, "sDJr": nrows * RS, "sJt": a["nseg"][nd - 1] * NPtot,
            "planeJd": nrows * NW, "planeI": ng * N, "planeJ": nrows * N}
    assert q == want
    # what a pass of this type touches, general and class-diagonal buffers alike
    ext = {"DI": nd * (q["sDIc"] + q["sDIr"]), "DJ": nd * (q["sDJc"] + q["sDJr"]), "Jrow": nd * q["sJd"], "Jt": nd * q["sJt"]}
    assert ext["DI"] == nd * ng * per_g >= 1 and ext["DJ"] == nd * nrows * per_g >= 1 and ext["Jrow"] >= 1 and ext["Jt"] >= 1
    assert q["DIr"] + nd * q["sDIr"] == ext["DI"] and q["DJr"] + nd * q["sDJr"] == ext["DJ"]      # row parts end where the region ends
    assert q["DI0"] + ext["DI"] <= P["DI"] == P["cd_DI"] and q["DJ0"] + ext["DJ"] <= P["DJ"] == P["cd_DJ"]
    assert ext["Jrow"] <= P["Jrow"] == P["cd_Jrow"] and ext["Jt"] <= P["Jt"]
    assert q["y0"] + nd * q["sy"] <= P["ypart"] and q["y0_cd"] + nd * q["sy"] <= P["cd_ypart"]


@pytest.mark.parametrize("rank", list(RANKS))
@pytest.mark.parametrize("tag", TAGS)
def test_regions_of_the_two_pass_types_are_disjoint(tag, rank):
    a = inputs(tag, rank)
    P = pt.jk_plan(**a)
    one, two = P["pass"][1], P["pass"][2]
    for buf, r in (("DI", "DIr"), ("DJ", "DJr")):
        end1 = one[buf + "0"] + one[r] + one["s" + r]                        # ND = 1: [column parts | row parts]
        assert one[buf + "0"] == 0 and end1 == two[buf + "0"], buf             # ND = 2 starts where ND = 1 ends ...
        assert two[buf + "0"] + two[r] + 2 * two["s" + r] == P[buf], buf       # ... and ends with the buffer
    # the class-diagonal ypart buffer: the ND = 2 region starts where the ND = 1 region ends, and fits
    assert one["y0_cd"] == 0 and two["y0_cd"] == one["y0_cd"] + one["sy"]
    assert two["y0_cd"] + 2 * two["sy"] <= P["cd_ypart"]
    # the general ypart buffer is shared: both pass types start at 0 and overwrite what they read
    assert one["y0"] == two["y0"] == 0
