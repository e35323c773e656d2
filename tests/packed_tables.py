"""TEST INFRASTRUCTURE: ctypes access to the host table builders of the packed tensor layout (tuna_amd/csrc/tf_packed_host.h),
compiled for the CPU by tests/packed_model/build.sh.  The tables are the library's own -- tf_build_eri uploads what these builders
make -- so tests can check them without a GPU (test_packed_tables.py) and pin the upload glue with one (test_gpu_packed_tables.py).
Nothing in the product imports this module."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

GROUP = np.dtype([("i", "i4"), ("j0", "i4"), ("nr", "i4"), ("r0", "i4"), ("c", "i4"), ("lamj0", "i4"), ("unr", "i4"), ("p0", "i4"),
                  ("ub", "i8"), ("secoff", "i4", 4)])
SUPER = np.dtype([("g0", "i4"), ("ng", "i4"), ("c", "i4"), ("i", "i4"), ("yoff", "i8"), ("ke", "i4", 4)])
TASK = np.dtype([("super", "i4"), ("w", "i4"), ("part", "i4"), ("pad", "i4")])
INT2 = np.dtype([("x", "i4"), ("y", "i4")])
KINFO = np.dtype([("offA", "i4"), ("cnt", "i4")])
_I8 = {"N", "NW", "RS", "MC", "KS", "MP", "NPtot", "RLS", "cbase", "NP", "pair_first_row", "rowoff", "n_elems", "nseg", "ypart_len",
       "class_row_off"}
_STRUCT = {"groups": GROUP, "supers": SUPER, "tasks": TASK, "tasks_cd": TASK, "row_ij": INT2, "jrows": INT2, "kinfo": KINFO}
_SCALAR = {"N", "NW", "RS", "MC", "KS", "MP", "NPtot", "RLS", "n_elems", "nseg", "ypart_len"}


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(HERE, "packed_model", "_build", "libpackedtables.so")
        csrc = os.path.join(HERE, "..", "tuna_amd", "csrc")
        src = [os.path.join(HERE, "packed_model", "packed_tables.cpp")] + [os.path.join(csrc, h) for h in
                                                                           ("tf_packed.h", "tf_packed_host.h", "tf_tiles.h", "tf_tiles_host.h", "tf_internal.h", "tf_jk_plan.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
            subprocess.check_call(["sh", os.path.join(HERE, "packed_model", "build.sh")])
        L = C.CDLL(so)
        L.ptm_build.restype = C.c_void_p
        L.ptm_build.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.ptm_free.argtypes = [C.c_void_p]
        L.ptm_error.restype = C.c_char_p
        L.ptm_error.argtypes = [C.c_void_p]
        L.ptm_const.restype = C.c_longlong
        L.ptm_const.argtypes = [C.c_char_p]
        L.ptm_get.restype = C.c_longlong
        L.ptm_get.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
        L.ptm_jk_plan.restype = C.c_longlong
        L.ptm_jk_plan.argtypes = [C.c_void_p, C.c_void_p]
        for name, dt in (("sizeof_JKGroup", GROUP), ("sizeof_JKSuper", SUPER), ("sizeof_JKTask", TASK)):
            assert L.ptm_const(name.encode()) == dt.itemsize, name
        _LIB = L
    return _LIB


def const(name):
    return int(lib().ptm_const(name.encode()))


class Tables:
    """the host tables of one build: cls[N] (original AO order), the AOs of every shell, the owned shell pairs (index A (A + 1) / 2 + B,
    A >= B; None: all), the parts of a cut walk and the rows of a group.  Every table of tf_packed_host.h by its member name."""

    def __init__(self, cls, shell_dim, my_pairs=None, parts=1, rb=8):
        L = lib()
        cls = np.ascontiguousarray(cls, dtype=np.int32)
        shell_dim = np.ascontiguousarray(shell_dim, dtype=np.int32)
        assert shell_dim.sum() == len(cls)
        ns = len(shell_dim)
        my_pairs = np.arange(ns * (ns + 1) // 2, dtype=np.int32) if my_pairs is None else np.ascontiguousarray(my_pairs, dtype=np.int32)
        h = L.ptm_build(len(cls), cls.ctypes.data, int(parts), ns, shell_dim.ctypes.data, len(my_pairs), my_pairs.ctypes.data, int(rb))
        try:
            err = L.ptm_error(h).decode()
            if err:
                raise RuntimeError(err)
            self._t = {}
            for name in ["N", "NW", "RS", "MC", "KS", "MP", "NPtot", "RLS", "cstart", "csize", "corder", "wfirst", "gbase", "cbase", "NP", "fullsec",
                         "cls", "loc", "sigma", "ao", "origI", "clsI", "cntA", "kap0", "kapF", "rpoff", "chunk_c0", "chunk_width", "chunk_cls",
                         "chunk_of", "gk", "kinfo", "offE", "row_ij", "rowmap", "pair_first_row", "rowoff", "rowsec", "rowlen", "n_elems",
                         "groups", "gfirst", "supers", "tasks", "tasks_cd", "bucket", "bucket_cd", "nseg", "ypart_len", "jp", "class_rows",
                         "row_pos", "class_row_off", "jptr", "jrows", "xorder"]:
                n = L.ptm_get(h, name.encode(), None)
                assert n >= 0, name
                a = np.zeros(n, dtype=_STRUCT.get(name, np.int64 if name in _I8 else np.int32))
                if n:
                    L.ptm_get(h, name.encode(), a.ctypes.data)
                self._t[name] = int(a[0]) if name in _SCALAR else a
        finally:
            L.ptm_free(h)

    def __getattr__(self, name):
        try:
            return self._t[name]
        except KeyError:
            raise AttributeError(name)


def group_table(T):
    """[n_groups][5] = (i, j0, nr, r0, c) of every group: what tf_debug_groups reports"""
    g = T.groups
    return np.stack([g["i"], g["j0"], g["nr"], g["r0"], g["c"]], axis=1).astype(np.int32) if len(g) else np.zeros((0, 5), np.int32)


PLAN_SIZES = ("Jrow", "ypart", "DI", "DJ", "Jt", "cd_Jrow", "cd_ypart", "cd_DI", "cd_DJ")
PLAN_PASS = ("DI0", "DJ0", "y0", "y0_cd", "DIr", "DJr", "sP", "sPp", "sy", "sJd", "sDIc", "sDIr", "sDJc", "sDJr", "sJt", "planeJd", "planeI", "planeJ")


def jk_plan(N, n_rows, NW, MP, RS, NPtot, n_groups, ypart_len, nseg):
    """the buffer plan of the packed Fock build (tuna_amd/csrc/tf_jk_plan.h) in doubles: {size name: doubles, "pass": {ND: {member: value}}};
    n_groups, ypart_len, nseg: per table set (set 0: one density per pass, set 1: two)"""
    arg = np.array([N, n_rows, NW, MP, RS, NPtot, *n_groups, *ypart_len, *nseg], dtype=np.int64)
    out = np.full(len(PLAN_SIZES) + 2 * len(PLAN_PASS), -1, dtype=np.int64)
    assert lib().ptm_jk_plan(arg.ctypes.data, out.ctypes.data) == len(out)
    plan = {k: int(v) for k, v in zip(PLAN_SIZES, out)}
    plan["pass"] = {nd: {k: int(v) for k, v in zip(PLAN_PASS, out[len(PLAN_SIZES) + (nd - 1) * len(PLAN_PASS):])} for nd in (1, 2)}
    return plan
