"""CPU: the plan of the symmetric eigensolver (tuna_amd/csrc/tf_eigh_plan.h, compiled with g++ through tests/eigh_plan_model).  The
refinement block's parts lie in the listed order without overlap, with the closed totals the eigensolver allocated before the layout
had a name, in 64 bits; the symmetry plan of a class vector (sizes, blocks, every word of the index table, the two predicates, the
work buffer's offsets) equals a restatement of the loop eigh_blocked had; the words of d_scal and of blk_ints do not overlap; the owner
of the grow-only blocks keeps, grows and drops as it says against an allocator that keeps books and refuses request k, for every k
(after a refusal the slot is null with capacity 0, every block is freed exactly once); EigState's two forget functions reset what they
name and no more.  The owner checks also run as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer where their
runtime is installed.  The header includes no HIP."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MODEL = os.path.join(HERE, "eigh_plan_model")
HEADER = os.path.join(HERE, "..", "tuna_amd", "csrc", "tf_eigh_plan.h")
PARTS = ("X", "Xn", "G", "Y", "S", "E", "lam", "wocc", "bmax", "homo_lumo", "vcls")                 # the listed order
NS = (1, 2, 15, 16, 17, 64, 65, 400, 2000)
# the class sizes of tests/test_gpu_eigh.py::CONFIGS, an empty class in the middle, a single class
SIZES = {"n39_below_nmin": (21, 8, 8, 2), "n40_blocked": (22, 8, 8, 2), "mmax64": (64, 24, 24, 0), "mmax65": (65, 24, 24, 0),
         "block_of_one": (36, 11, 11, 1), "one_class_dominates": (62, 2, 2, 0), "empty_middle": (5, 0, 3, 2), "single_class": (0, 0, 9, 0)}
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(MODEL, "_build", "libeighplan.so")
        src = [os.path.join(MODEL, f) for f in ("eigh_plan.cpp", "owner_checks.h", "owner_main.cpp", "build.sh")] + [HEADER]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
            subprocess.check_call(["sh", os.path.join(MODEL, "build.sh")])
        L = C.CDLL(so)
        L.eighm_ref_layout.argtypes = [C.c_int, C.c_void_p]
        L.eighm_sym_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong]
        L.eighm_ints.argtypes = [C.c_void_p]
        L.eighm_scal_words.argtypes = [C.c_void_p]
        L.eighm_owner_ops.argtypes = [C.c_void_p]
        L.eighm_owner.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        L.eighm_state.argtypes = [C.c_void_p]
        _LIB = L
    return _LIB


# ---- RefLayout ----------------------------------------------------------------------------------------------------------------------
def ref_layout(n):
    out = np.zeros(13, dtype=np.int64)
    lib().eighm_ref_layout(n, out.ctypes.data)
    return dict(zip(PARTS + ("total", "npin"), (int(x) for x in out)))


def check_ref_layout(n):
    L = ref_layout(n)
    nn, g = n * n, (n * n + 255) // 256
    length = {"X": nn, "Xn": nn, "G": nn, "Y": nn, "S": nn, "E": nn, "lam": n, "wocc": n, "bmax": 2 * g, "homo_lumo": 2, "vcls": (4 * n + 7) // 8}
    spans = [(L[p], L[p] + length[p]) for p in PARTS]
    assert spans[0][0] == 0 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (n, spans)     # in the listed order, disjoint
    assert all(a[1] == b[0] for a, b in zip(spans[:9], spans[1:10]))                                # X ... homo_lumo without a gap
    assert 8 * L["vcls"] + 4 * n <= 8 * L["total"]                                                  # n ints of labels end inside
    assert L["total"] == 6 * nn + 3 * n + 2 * g + 8 and L["vcls"] == 6 * nn + 2 * n + 2 * g + 8 and L["npin"] == 2 * g + 2
    assert L["homo_lumo"] + 2 - L["bmax"] == L["npin"]                                              # what one read-back fetches
    return L


@pytest.mark.parametrize("n", NS)
def test_ref_layout_is_ordered_disjoint_and_has_the_closed_totals(n):
    check_ref_layout(n)


def test_ref_layout_in_64_bits():
    L = check_ref_layout(50_000)
    assert L["total"] > 2 ** 33 and L["E"] == 5 * 50_000 ** 2 > 2 ** 31


# ---- SymPlan ------------------------------------------------------------------------------------------------------------------------
def class_vector(sizes, seed=0):
    cls = np.repeat(np.arange(4), sizes).astype(np.int32)
    return np.ascontiguousarray(np.random.default_rng(seed).permutation(cls))


def sym_plan(cls):
    cls = np.ascontiguousarray(cls, dtype=np.int32)
    hdr, idx = np.full(22, -7, dtype=np.int64), np.full(4 * len(cls) + len(cls) + 4 + 8, -7, dtype=np.int32)
    ok = lib().eighm_sym_plan(cls.ctypes.data, len(cls), hdr.ctypes.data, idx.ctypes.data, len(idx))
    keys = ("n", "nb", "mmax") + tuple(f"m{k}" for k in range(4)) + tuple(f"blk_of{k}" for k in range(4)) + (
        "worth", "lds", "idx_cls", "idx_sizes", "idx_len", "blocks_len", "B", "D", "E", "flag", "buf_len")
    p = dict(zip(keys, (int(x) for x in hdr)))
    p["idx"] = [int(x) for x in idx[:p["idx_len"]]]
    assert all(x == -7 for x in idx[p["idx_len"]:])                                                 # nothing written behind the table
    return ok, p


def restated_tables(cls):
    """the loop eigh_blocked had, word for word"""
    n = len(cls)
    m = [0, 0, 0, 0]
    for c in cls:
        m[c] += 1
    nb, mmax, blk_of, sym_m = 0, 0, [-1] * 4, [0] * 4
    for c in range(4):
        if m[c] > 0:
            blk_of[c] = nb
            sym_m[nb] = m[c]
            nb += 1
            mmax = max(mmax, m[c])
    idx = [-1] * (4 * mmax + n + 4)
    fill = [0] * 4
    for i in range(n):
        b = blk_of[cls[i]]
        idx[b * mmax + fill[b]] = i
        fill[b] += 1
        idx[4 * mmax + i] = int(cls[i])
    for b in range(4):
        idx[4 * mmax + n + b] = sym_m[b] if b < nb else 0
    return nb, mmax, blk_of, sym_m, idx


@pytest.mark.parametrize("name", sorted(SIZES))
def test_sym_plan_is_the_loop_it_replaces(name):
    for seed in (0, 1):
        cls = class_vector(SIZES[name], seed)
        ok, p = sym_plan(cls)
        nb, mmax, blk_of, sym_m, idx = restated_tables(cls)
        n = len(cls)
        assert ok == 1 and (p["n"], p["nb"], p["mmax"]) == (n, nb, mmax)
        assert [p[f"m{k}"] for k in range(4)] == sym_m and [p[f"blk_of{k}"] for k in range(4)] == blk_of
        assert p["idx"] == idx                                                                      # every word of the index table
        assert (p["idx_cls"], p["idx_sizes"], p["idx_len"]) == (4 * mmax, 4 * mmax + n, 4 * mmax + n + 4)
        assert p["worth"] == int(nb >= 2 and 4 * mmax <= 3 * n) and p["lds"] == int(mmax <= 64)
        # the work buffer: B [nb][mmax][mmax] | D [nb][mmax] | E [nb][mmax] | flag (4 doubles), as eigh_blocked allocated and carved it
        assert p["blocks_len"] == nb * mmax * mmax
        assert (p["B"], p["D"], p["E"], p["flag"]) == (0, nb * mmax * mmax, nb * mmax * mmax + nb * mmax, nb * mmax * mmax + 2 * nb * mmax)
        assert p["buf_len"] == nb * mmax * mmax + 2 * nb * mmax + 4
    assert p["worth"] == (0 if name in ("one_class_dominates", "single_class") else 1)
    assert p["lds"] == (0 if name == "mmax65" else 1)


def test_sym_plan_of_the_named_cases():
    _, p = sym_plan(class_vector(SIZES["empty_middle"]))
    assert (p["nb"], p["mmax"]) == (3, 5) and [p[f"blk_of{k}"] for k in range(4)] == [0, -1, 1, 2] and [p[f"m{k}"] for k in range(4)] == [5, 3, 2, 0]
    _, p = sym_plan(class_vector(SIZES["single_class"]))
    assert (p["nb"], p["mmax"], p["worth"]) == (1, 9, 0) and p["idx"][:9] == list(range(9))
    _, p = sym_plan(class_vector(SIZES["mmax64"]))
    assert (p["nb"], p["mmax"], p["lds"], p["worth"]) == (3, 64, 1, 1)


@pytest.mark.parametrize("bad", (4, -1))
def test_sym_plan_refuses_a_class_outside_0_to_3(bad):
    cls = class_vector((5, 4, 3, 2))
    cls[7] = bad
    ok, p = sym_plan(cls)
    assert ok == 0 and (p["n"], p["nb"], p["mmax"]) == (0, 0, 0)                                    # refused, and no plan made


# ---- the words of blk_ints and d_scal -------------------------------------------------------------------------------------------------
def test_blk_ints_words():
    out = np.zeros(7, dtype=np.int64)
    lib().eighm_ints(out.ctypes.data)
    nocc0, nocc1, status, combined, length, lds, nblocks = (int(x) for x in out)
    assert (nocc0, status, combined, nocc1, length) == (0, 4, 12, 16, 32)                           # the numbers the kernels' callers used
    spans = sorted([(nocc0, nocc0 + 4), (status, status + 8), (combined, combined + 2), (nocc1, nocc1 + 4)])
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= length
    assert lds == 64 and nblocks == 12


def test_d_scal_words_do_not_overlap():
    out = np.zeros(25, dtype=np.int64)
    npairs = lib().eighm_scal_words(out.ctypes.data)
    pairs = [(int(out[2 * k]), int(out[2 * k + 1])) for k in range(npairs)]
    # DESIGN.md 4.4a invariant 3, restated: populations 0...7; density changes 16, 17; energy terms 18...22 and 24...28; the solver status
    # at 23 and 30; history dots from 128, second spin from 192; the eigensolver's words 32, 40, 48, 62
    assert pairs == [(0, 8), (16, 2), (18, 5), (24, 5), (23, 1), (30, 1), (32, 1), (40, 1), (48, 1), (62, 1), (128, 64), (192, 64)]
    spans = sorted((a, a + n) for a, n in pairs)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans
    assert spans[-1][1] == int(out[24]) == 256
    assert 16 + 8 > 23 and 16 + 15 > 30                                                             # the cycles' read-backs of 8 and 15 doubles reach the status words


# ---- Blocks<N> ------------------------------------------------------------------------------------------------------------------------
def owner_ops():
    ops = np.zeros(3 * 64, dtype=np.int64)
    n = lib().eighm_owner_ops(ops.ctypes.data)
    return [tuple(int(x) for x in ops[3 * i:3 * i + 3]) for i in range(n)]


def owner(k, nops):
    per_op, totals = np.zeros(6 * nops, dtype=np.int64), np.zeros(8, dtype=np.int64)
    verdict = lib().eighm_owner(k, per_op.ctypes.data, totals.ctypes.data)
    keys = ("requests", "handed", "live", "freed", "bad_frees", "leaked", "left_in_table", "freed_after_second_release")
    return verdict, per_op.reshape(nops, 6).tolist(), dict(zip(keys, (int(x) for x in totals)))


def model(ops, k, refused):
    """what ensure and drop promise: (code, requests so far, non-null, capacity, frees so far) per operation"""
    cap, requests, frees, rows = {}, 0, 0, []
    for kind, slot, nbytes in ops:
        rc, had = 0, cap.get(slot, 0) > 0
        if kind == 1:
            frees += had
            cap[slot] = 0
        elif not (had and cap[slot] >= nbytes):
            frees += had                                                                            # freed once, before the request
            cap[slot] = 0
            if requests == k:
                rc = refused
            else:
                cap[slot] = nbytes
            requests += 1
        rows.append((rc, requests, int(cap[slot] > 0), cap[slot], frees))
    return rows, cap


def test_owner_sequence_touches_every_slot_and_every_kind_of_request():
    ops = owner_ops()
    rows, _ = model(ops, -1, 0)
    assert {s for _, s, _ in ops} == {0, 1, 2, 3}
    requested = [i for i in range(len(ops)) if rows[i][1] > (rows[i - 1][1] if i else 0)]
    kept = [i for i, (kind, _, _) in enumerate(ops) if kind == 0 and i not in requested]
    assert any(ops[i][2] == rows[i][3] for i in kept) and any(ops[i][2] < rows[i][3] for i in kept)   # an equal and a smaller request are kept
    assert any(rows[i][4] > rows[i - 1][4] for i in requested if i)                                 # a request that replaces a block


def test_owner_at_every_refusal_position():
    ops = owner_ops()
    refused = lib().eighm_refused()
    n_requests = model(ops, -1, refused)[0][-1][1]
    assert n_requests >= 8
    for k in range(-1, n_requests):
        verdict, per_op, t = owner(k, len(ops))
        rows, cap = model(ops, k, refused)
        assert verdict == 0, (k, verdict)                                                           # the C++ restatement (the stand-alone program's)
        for i, (row, got) in enumerate(zip(rows, per_op)):
            assert tuple(got[:4]) + (got[5],) == row, (k, i, ops[i], got, row)
            if ops[i][0] == 0 and row[1] == (rows[i - 1][1] if i else 0):
                assert got[4] == 1, (k, i)                                                          # kept: the same block
            if row[0] != 0:
                assert got[2] == 0 and got[3] == 0                                                  # refused: null with capacity 0
        made = rows[-1][1]                                                                          # (a slot emptied by a refusal asks again later)
        handed = made - (1 if k >= 0 else 0)
        assert sum(1 for r in rows if r[0] != 0) == (1 if k >= 0 else 0) and made >= n_requests
        assert t["requests"] == made and t["handed"] == handed and t["live"] == sum(1 for v in cap.values() if v)
        assert t["freed"] == handed and t["bad_frees"] == 0 and t["leaked"] == 0 and t["left_in_table"] == 0
        assert t["freed_after_second_release"] == handed                                            # a second release frees nothing


# ---- EigState -------------------------------------------------------------------------------------------------------------------------
def test_state_forgets_what_it_names_and_frees_each_block_once():
    out = np.zeros(30, dtype=np.int64)
    assert lib().eighm_state(out.ctypes.data) == 0
    keys = ("sym_n", "sym_prev_n", "blk_n0", "blk_n1", "ref_n0", "ref_n1", "vcls_n0", "vcls_n1", "jac_prev_n")
    tables, vectors = dict(zip(keys, out[:9].tolist())), dict(zip(keys, out[9:18].tolist()))
    assert tables == dict(sym_n=0, sym_prev_n=0, blk_n0=0, blk_n1=0, ref_n0=7, ref_n1=7, vcls_n0=7, vcls_n1=7, jac_prev_n=7)
    assert vectors == dict(sym_n=7, sym_prev_n=7, blk_n0=0, blk_n1=0, ref_n0=0, ref_n1=0, vcls_n0=0, vcls_n1=0, jac_prev_n=7)
    assert int(out[18]) == 1                                                                        # the current spin is not theirs to change
    spin0, spin1 = out[19:22].tolist(), out[22:25].tolist()
    assert spin0[2] == 0 and spin1[2] == 16 and len({spin0[0], spin0[1], spin1[0], spin1[1]}) == 4  # no block shared between the spins
    handed, freed, bad, leaked, freed_again = out[25:30].tolist()
    assert handed == 13 and freed == 13 and bad == 0 and leaked == 0 and freed_again == 13          # twelve device blocks and the pinned one


def test_owner_checks_as_a_program_of_their_own():
    """tests/eigh_plan_model/owner_main.cpp: with -fsanitize=address,undefined where build.sh found the runtime"""
    lib()
    exe = os.path.join(MODEL, "_build", "owner_main")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr, "sanitized" if os.path.exists(exe + ".sanitized") else "built without the sanitizers")
    assert p.returncode == 0 and "0 failed" in p.stdout, p.stdout + p.stderr


def test_header_includes_no_hip():
    text = open(HEADER).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<cstddef>", "<vector>"], includes
    assert "hip" not in " ".join(includes).lower() and "__global__" not in text and "rocblas_" not in text and "hipMalloc" not in text
