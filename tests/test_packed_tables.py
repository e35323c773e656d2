"""CPU: the host tables of the packed tensor layout as the library builds them (tuna_amd/csrc/tf_packed_host.h, compiled with g++ by
tests/packed_model/build.sh) -- the layout tables against the independent NumPy model tests/layout_model.py, and the structure of
the row tables, storage units, work tables of the Fock kernel and reduction lists that the kernels rely on."""
import numpy as np
import pytest

import layout_model as lm
import packed_tables as pt

SPH_CLASSES = {0: [0], 1: [1, 2, 0], 2: [3, 1, 2, 0, 0], 3: [2, 3, 2, 0, 1, 0, 1]}     # parity class of every real harmonic, reference order
SHELL_LISTS = [[0, 0, 1, 2, 1, 0, 2, 3, 1, 0], [0, 1, 1, 2, 0, 1, 2, 2, 3, 0, 1], [0, 0, 0, 0], [1, 0, 2],      # (test_layout_model.py, test_tile_model.py)
               [0] * 140 + [1] * 5]       # 145 AOs in class 0: three column chunks, the last one partial


def classes_of(shell_L):
    out = []
    for L in shell_L:
        out += SPH_CLASSES[L]
    return out


def shell_dims(shell_L):
    return [2 * L + 1 for L in shell_L]


def owned_pairs(shell_L, split):
    """split None: one rank; (rank, 2): every other shell pair goes to rank 1"""
    ns = len(shell_L)
    allp = np.arange(ns * (ns + 1) // 2)
    return None if split is None else allp[allp % 2 == split[0]]


@pytest.mark.parametrize("shell_L", SHELL_LISTS, ids=lambda s: f"{len(s)}shells")
def test_layout_tables_equal_the_independent_model(shell_L):
    cls = classes_of(shell_L)
    assert pt.const("SEG_PAD") == lm.PAD and pt.const("CW") == lm.CW
    T = pt.Tables(cls, shell_dims(shell_L))
    L = lm.Layout(cls)
    N = T.N
    assert N == L.N and T.NW == L.NW and T.NPtot == L.NPtot
    if shell_L == SHELL_LISTS[-1]:
        assert T.csize.max() >= 130 and list(T.chunk_width[T.chunk_cls == 0]) == [64, 64, 17]
    for mine, model in (("cstart", L.cstart), ("csize", L.csize), ("corder", L.corder), ("loc", L.loc), ("sigma", L.sigma), ("origI", L.orig),
                        ("clsI", L.clsI), ("NP", L.NP), ("cbase", L.cbase), ("chunk_cls", L.chunk_cls), ("chunk_c0", L.chunk_c0),
                        ("chunk_width", L.chunk_width), ("chunk_of", L.chunk_of), ("wfirst", L.wfirst)):
        np.testing.assert_array_equal(getattr(T, mine), np.asarray(model), err_msg=mine)
    kinfo = T.kinfo.reshape(4, N)
    np.testing.assert_array_equal(kinfo["cnt"], L.cntI)
    np.testing.assert_array_equal(kinfo["offA"], L.offA)
    np.testing.assert_array_equal(T.offE.reshape(4, N), L.offE)
    np.testing.assert_array_equal(T.fullsec.reshape(4, 4), L.fullsec)
    np.testing.assert_array_equal(T.kap0[:4 * T.NW].reshape(4, T.NW), L.kap0)
    for c in range(4):
        np.testing.assert_array_equal(T.gk[T.gbase[c]: T.gbase[c] + T.NP[c] // lm.PAD], L.gk[c])
    # every row: its length and section starts
    assert len(T.row_ij) == N * (N + 1) // 2
    per_i = {}
    for r, (i, j) in enumerate(zip(T.row_ij["x"], T.row_ij["y"])):
        c = int(L.cls[i] ^ L.cls[j])
        if (c, i) not in per_i:
            per_i[(c, i)] = L.secoff(c, i)
        secoff, tot = per_i[(c, i)]
        assert T.rowlen[r] == tot == L.row_len(i, j) and list(T.rowsec[6 * r: 6 * r + 4]) == secoff


def check_structure(shell_L, split, rb, parts):
    cls = classes_of(shell_L)
    T = pt.Tables(cls, shell_dims(shell_L), owned_pairs(shell_L, split), parts, rb)
    L = lm.Layout(cls)
    N, NW = T.N, T.NW
    sig = T.sigma
    rows = list(zip(T.row_ij["x"].tolist(), T.row_ij["y"].tolist()))
    n_rows = len(rows)
    # the owned rows are those of the owned shell pairs, in ascending internal (i, j); rowmap finds them
    off = np.concatenate([[0], np.cumsum(shell_dims(shell_L))])
    ns = len(shell_L)
    mine = owned_pairs(shell_L, split)
    mine = set(range(ns * (ns + 1) // 2)) if mine is None else set(mine.tolist())
    want = {(i, j) for A in range(ns) for B in range(A + 1) if A * (A + 1) // 2 + B in mine
            for i in range(off[A], off[A + 1]) for j in range(off[B], off[B + 1]) if i >= j}
    assert set(rows) == want and len(want) == n_rows
    keys = [sig[i] * N + sig[j] for i, j in rows]
    assert keys == sorted(keys)
    for r, (i, j) in enumerate(rows):
        assert T.rowmap[L.key(int(sig[i]), int(sig[j]))] == r
    assert (T.rowmap >= 0).sum() == n_rows
    # groups: every owned row in exactly one; at most RB rows, one i, one class, consecutive internal j
    G = T.groups
    seen = np.zeros(n_rows, dtype=int)
    for g in G:
        assert 1 <= g["nr"] <= rb
        for k in range(g["nr"]):
            i, j = rows[g["r0"] + k]
            seen[g["r0"] + k] += 1
            assert sig[i] == g["i"] and sig[j] == g["j0"] + k and T.clsI[sig[j]] == T.clsI[g["j0"]]
        assert g["c"] == T.clsI[g["i"]] ^ T.clsI[g["j0"]] and g["lamj0"] == g["j0"] - T.cstart[T.clsI[g["j0"]]]
    assert np.all(seen == 1)
    # gfirst brackets the groups of each i
    for a in range(N):
        idx = np.nonzero(G["i"] == a)[0]
        if len(idx):
            assert list(idx) == list(range(T.gfirst[a], T.gfirst[N + a]))
        else:
            assert T.gfirst[a] == T.gfirst[N + a]
    # supers: every group in exactly one, at most GPW * W groups of one i and class; ordered by (class, descending original i)
    S = T.supers
    gseen = np.zeros(len(G), dtype=int)
    for s in S:
        assert 1 <= s["ng"] <= pt.const("GPW") * pt.const("W")
        for gi in range(s["g0"], s["g0"] + s["ng"]):
            gseen[gi] += 1
            assert G[gi]["i"] == s["i"] and G[gi]["c"] == s["c"]
        assert list(s["ke"]) == [L.ke(a, int(T.origI[s["i"]])) for a in range(4)]
    assert np.all(gseen == 1)
    order = [(int(s["c"]), -int(T.origI[s["i"]])) for s in S]
    assert order == sorted(order)
    # tasks: exactly {(super, chunk, part) : the task exists and part KS < walk}
    longest = max(1, int(T.csize.max()))
    MP = max(1, min(parts, longest))
    KS = (longest + MP - 1) // MP
    assert (T.MP, T.KS) == (MP, KS)
    want_tasks = set()
    for si, s in enumerate(S):
        c, io = int(s["c"]), int(T.origI[s["i"]])
        for w in range(NW):
            if L.task_exists(c, w, io):
                walk = L.ke(L.chunk_cls[w] ^ c, io) - int(L.kap0[c][w])
                want_tasks |= {(si, w, part) for part in range((walk + KS - 1) // KS)}
    tasks = [(int(t["super"]), int(t["w"]), int(t["part"])) for t in T.tasks]
    assert len(tasks) == len(set(tasks)) and set(tasks) == want_tasks
    # buckets; the class-diagonal list is the subsequence with c == 0 or the chunk's class in {class(i), class(j)}
    b = list(T.bucket)
    assert b[0] == 0 and b[3] == len(tasks) and b == sorted(b)
    def diagonal(t):
        s = S[t[0]]
        ci = int(T.clsI[s["i"]])
        return s["c"] == 0 or int(T.chunk_cls[t[1]]) in (ci, ci ^ int(s["c"]))
    keep = [diagonal(t) for t in tasks]
    cd = [(int(t["super"]), int(t["w"]), int(t["part"])) for t in T.tasks_cd]
    assert cd == [t for t, k in zip(tasks, keep) if k]
    assert list(T.bucket_cd) == [int(np.sum(keep[:b[q]])) for q in range(4)]
    # storage units tile [0, n_elems); n_elems is the sum of the row lengths
    units = {}
    for r in range(n_rows):
        units.setdefault(int(T.rowoff[r]), []).append(r)
    pos = 0
    for ub in sorted(units):
        rs = units[ub]
        assert ub == pos and [int(T.rowsec[6 * r + 4]) for r in rs] == list(range(len(rs))) and all(T.rowsec[6 * r + 5] == len(rs) for r in rs)
        assert len(rs) <= pt.const("JBB") and len({int(T.rowlen[r]) for r in rs}) == 1
        pos += len(rs) * int(T.rowlen[rs[0]])
    assert pos == T.n_elems == T.rowoff[n_rows] == sum(L.row_len(i, j) for i, j in rows)
    for g in G:       # a group lies inside one unit
        assert g["ub"] == T.rowoff[g["r0"]] == T.rowoff[g["r0"] + g["nr"] - 1] and g["p0"] == T.rowsec[6 * g["r0"] + 4] and g["unr"] == T.rowsec[6 * g["r0"] + 5]
    # reduction lists: every off-diagonal owned row once under its second index, ascending; xorder a permutation
    assert T.jptr[0] == 0 and len(T.jptr) == N + 1
    for x in range(N):
        got = [(int(e["x"]), int(e["y"])) for e in T.jrows[T.jptr[x]: T.jptr[x + 1]]]
        assert got == [(r, i) for r, (i, j) in enumerate(rows) if sig[j] == x and sig[i] != x]
    assert T.jptr[N] == sum(1 for i, j in rows if i != j)
    assert sorted(T.xorder.tolist()) == list(range(N))
    # rows by class
    assert sorted(T.class_rows.tolist()) == list(range(n_rows)) and T.class_row_off[4] == n_rows
    for c in range(4):
        for q in range(T.class_row_off[c], T.class_row_off[c + 1]):
            i, j = rows[T.class_rows[q]]
            assert L.cls[i] ^ L.cls[j] == c and T.row_pos[T.class_rows[q]] == q


@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("rb", [8, 4])
@pytest.mark.parametrize("split", [None, (0, 2), (1, 2)], ids=["world1", "rank0of2", "rank1of2"])
@pytest.mark.parametrize("shell_L", SHELL_LISTS[:4], ids=lambda s: f"{len(s)}shells")
def test_table_structure(shell_L, split, rb, parts):
    check_structure(shell_L, split, rb, parts)


@pytest.mark.parametrize("split,rb,parts", [(None, 8, 1), ((1, 2), 4, 3), ((0, 2), 8, 3), (None, 4, 1)])
def test_table_structure_three_chunks_in_a_class(split, rb, parts):
    check_structure(SHELL_LISTS[-1], split, rb, parts)
