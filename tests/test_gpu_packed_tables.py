"""GPU (MI355X): the upload glue of the packed layout's work tables -- tf_debug_groups returns the row groups that sit on the device;
they must be exactly the groups the host builders of tuna_amd/csrc/tf_packed_host.h (compiled for the CPU, tests/packed_tables.py)
make for the same AO classes and owned rows."""
import ctypes as C

import numpy as np
import pytest

import packed_tables as pt
from conftest import make_system
from tuna_amd import distributed as dist
from tuna_amd.engine import Engine

pytestmark = pytest.mark.gpu


def device_groups(eng):
    L = eng._L
    L.tf_debug_groups.restype = C.c_int
    L.tf_debug_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    n = L.tf_debug_groups(eng._ctx, None, 0)
    assert n >= 0
    out = np.zeros((n, 5), dtype=np.int32)
    assert L.tf_debug_groups(eng._ctx, out.ctypes.data, n) == n
    return out


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
@pytest.mark.parametrize("tag", ["n2_sto3g", "c4_co_def2tzvp"])
def test_device_groups_are_the_host_builders(tag, rank, world):
    atoms, shells, aos, _ = make_system(tag)
    with Engine(0, rank, world) as eng:
        eng.set_basis(aos).build_eri(True, layout="packed")
        assert eng.eri_storage()["layout"] == "packed"
        got = device_groups(eng)
        U = eng.sph_matrix()
    # parity class of a real spherical AO: that of its first Cartesian component
    first = np.argmax(U != 0.0, axis=1)
    cls = (aos.lmn[first, 0] & 1) | ((aos.lmn[first, 1] & 1) << 1)
    owner = dist.shard_owner(shells, world, True, "packed")
    parts = 4 if world >= 4 else (2 if world >= 2 else 1)
    T = pt.Tables(cls, [s.n_sph for s in shells], np.nonzero(owner == rank)[0], parts, pt.const("RB1"))
    want = pt.group_table(T)
    assert len(want) > 0 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
