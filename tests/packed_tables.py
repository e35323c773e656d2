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
                                                                           ("tf_packed.h", "tf_packed_host.h", "tf_tiles.h", "tf_tiles_host.h", "tf_internal.h", "tf_jk_plan.h", "tf_eri_types.h", "tf_eri_plan.h")]
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


# ---- the LDS plans of the ERI kernels (tuna_amd/csrc/tf_eri_plan.h): integers in, the members of the launch record out ----------
ERI_Q_FIELDS = ("offR", "offPref", "offPQ", "offRed", "offEab", "offEcd", "offScale", "offLmn", "offBlk", "offG", "offTab", "offCsr", "lds_doubles",
                "PB", "stride", "G", "ncp", "tupG_off", "tupXZ_off", "stage")
ERI_FAMILY = {"multi": 0, "fact": 1, "class": 2, "component_lane": 3}
ERI_CF_FIELDS = ("offR", "capR", "offPref", "offPQ", "offPP", "offG", "capG", "offX", "offZ", "capXZ", "offTupG", "offTupXZ", "offEab", "capEab",
                 "offEcd", "capEcd", "offRed", "lds_doubles", "tri", "gtab_doubles", "dbg_npq_lo", "dbg_npq_hi", "offKm", "capKm", "team_lmax",
                 "team_pqmax", "fit", "gtab")
ERI_LREC_FIELDS = ("L", "nM", "tsize", "nT", "xz", "gsz", "lgG", "lgX", "nb_cap", "tupG_off", "tupXZ_off", "pad")
ERI_TEAM_FIELDS = ("oE12", "oOffA", "oScA", "oOffK", "oTp", "oTk", "oTc", "oRowOff", "oCompW", "oOutW", "flat_off", "nflat")
ERI_TEAM_SIZE_FIELDS = ("vcap", "team_doubles", "shared_doubles", "flat", "bytes")
_ERI_READY = False


def _eri():
    global _ERI_READY
    L = lib()
    if not _ERI_READY:
        vp, ci, ll = C.c_void_p, C.c_int, C.c_longlong
        L.ptm_eri_carve.restype = ll; L.ptm_eri_carve.argtypes = [ci, vp, ci, ci, vp]
        L.ptm_eri_lp_group.restype = ci; L.ptm_eri_lp_group.argtypes = [ci]
        L.ptm_eri_group_stat.restype = None; L.ptm_eri_group_stat.argtypes = [ci, vp, vp]
        L.ptm_eri_cfact.restype = ll; L.ptm_eri_cfact.argtypes = [vp, vp]
        L.ptm_eri_lrec.restype = ll; L.ptm_eri_lrec.argtypes = [vp, ci, vp, vp, vp]
        L.ptm_eri_team.restype = ll; L.ptm_eri_team.argtypes = [ci, vp, vp]
        L.ptm_eri_choose_team.restype = ci; L.ptm_eri_choose_team.argtypes = [vp, vp, ci, ci, ll, ci, ci]
        L.ptm_eri_team_grid_x.restype = ll; L.ptm_eri_team_grid_x.argtypes = [ci, ci, ll, ll, ll]
        _ERI_READY = True
    return L


def eri_carve(family, cases, tupG=0, tupXZ=0):
    """cases[n][10] = La Lb Lc Ld nca ncb ncc ncd npp_ab npp_cd -> {member: int64[n]} of the QClass the family's carve function fills"""
    L, fam = _eri(), ERI_FAMILY[family]
    cases = np.ascontiguousarray(cases, dtype=np.int32)
    out = np.zeros((len(cases), len(ERI_Q_FIELDS)), dtype=np.int32)
    for k in range(len(cases)):
        assert L.ptm_eri_carve(fam, cases[k].ctypes.data, tupG, tupXZ, out[k].ctypes.data) == len(ERI_Q_FIELDS)
    return {f: out[:, i].astype(np.int64) for i, f in enumerate(ERI_Q_FIELDS)}


def eri_lp_group(lp):
    return int(_eri().ptm_eri_lp_group(int(lp)))


def eri_group_stat(pairs):
    """pairs[n][5] = La Lb npp nE component pairs -> (maxLp, maxT, maxLp1, maxE, maxcomp, maxnpp)"""
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 5)
    out = np.zeros(6, dtype=np.int32)
    _eri().ptm_eri_group_stat(len(pairs), pairs.ctypes.data, out.ctypes.data)
    return tuple(int(v) for v in out)


def eri_cfact(cases):
    """cases[n][21] = GroupStat bra, GroupStat ket, bra contracted, ket contracted, nbt, xz, e, km members, packed, team_lmax, team_pqmax"""
    L = _eri()
    cases = np.ascontiguousarray(cases, dtype=np.int32)
    out = np.zeros((len(cases), len(ERI_CF_FIELDS)), dtype=np.int32)
    for k in range(len(cases)):
        assert L.ptm_eri_cfact(cases[k].ctypes.data, out[k].ctypes.data) == len(ERI_CF_FIELDS)
    return {f: out[:, i].astype(np.int64) for i, f in enumerate(ERI_CF_FIELDS)}


def eri_lrec(L4, caps=()):
    """(La, Lb, Lc, Ld), [(capR, capG, capXZ), ..] -> ({member: int}, the gsz G words and xz X/Z words)"""
    L4 = np.ascontiguousarray(L4, dtype=np.int32)
    caps = np.ascontiguousarray(caps, dtype=np.int32).reshape(-1, 3)
    out = np.zeros(len(ERI_LREC_FIELDS), dtype=np.int32)
    n = _eri().ptm_eri_lrec(L4.ctypes.data, len(caps), caps.ctypes.data, out.ctypes.data, None)
    words = np.zeros(n, dtype=np.uint16)
    _eri().ptm_eri_lrec(L4.ctypes.data, len(caps), caps.ctypes.data, out.ctypes.data, words.ctypes.data)
    return {f: int(v) for f, v in zip(ERI_LREC_FIELDS, out)}, words


def eri_team(per_class, cases):
    """cases[n][16] = La Lb Lc Ld nab ncd nkap nnzT nacc nout foff maxblk maxK nnzc nEab nEcd -> {member: int64[n]}, per-size members
    as member_16 / _64 / _256"""
    L = _eri()
    cases = np.ascontiguousarray(cases, dtype=np.int32)
    nf = len(ERI_TEAM_FIELDS) + 3 * len(ERI_TEAM_SIZE_FIELDS)
    out = np.zeros((len(cases), nf), dtype=np.int64)
    for k in range(len(cases)):
        assert L.ptm_eri_team(int(per_class), cases[k].ctypes.data, out[k].ctypes.data) == nf
    names = list(ERI_TEAM_FIELDS) + [f"{f}_{tm}" for tm in (16, 64, 256) for f in ERI_TEAM_SIZE_FIELDS]
    return {f: out[:, i] for i, f in enumerate(names)}


def eri_choose_team(avail, nbytes, nT, nnzc, soft64, t16_nnz, force):
    a, b = np.ascontiguousarray(avail, dtype=np.int32), np.ascontiguousarray(nbytes, dtype=np.int64)
    return int(_eri().ptm_eri_choose_team(a.ctypes.data, b.ctypes.data, int(nT), int(nnzc), int(soft64), int(t16_nnz), int(force)))


def eri_team_grid_x(n_ket, team, n_bra, kpw_div, kpw_max):
    return int(_eri().ptm_eri_team_grid_x(int(n_ket), int(team), int(n_bra), int(kpw_div), int(kpw_max)))
