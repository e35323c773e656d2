"""CPU: the LDS plans of the ERI kernels (tuna_amd/csrc/tf_eri_plan.h, compiled with g++ through tests/packed_model) against the sizes the
kernel headers require of every region, written out here in NumPy integers.  Range: (La, Lb | Lc, Ld) in 0 .. 5, primitive-pair depths
1, 2, 8 and 13, spherical and Cartesian output (the team kernels: the only records that depend on it), and for eri_cfact_kernel every
pair of the fourteen pair groups with the group maxima of the basis sets of tests/eri_shapes.py (high_l among them) and of every single
(La, Lb, depth).  Per carve function: the regions, in declaration order, start where the previous one ended (but for the documented
aliases), lds_doubles is the end of the last one, every region is at least as large as the kernel needs, `fit` is bytes <=
ERI_LDS_MAX_BYTES, a global-table plan exists only for uncontracted group pairs that do not fit.  The team-size choice against its
rules and against a table of cases written out by hand from the two cascades it replaced; nb_cap against the caps it came from; the
index words decoded back to their loop indices."""
import itertools

import numpy as np
import pytest

import eri_shapes as es
import packed_tables as pt

THREADS, BLK, CSR, LDS_MAX = (pt.const(n) for n in ("ERI_THREADS", "BLK_DOUBLES", "CSR_DOUBLES", "ERI_LDS_MAX_BYTES"))
DEPTHS = (1, 2, 8, 13)
L4 = np.array(list(itertools.product(range(6), repeat=4)), dtype=np.int64)
SYSTEM_TAGS = ("one_p", "deep_p", "f_mix", "n2_ccpvdz", "c2_n2_ccpvtz", "high_l")


def ncart(L):
    return (L + 1) * (L + 2) // 2


def nE(La, Lb):
    return (La + 1) * (Lb + 1) * (La + Lb + 1)


def q_cases(depths):
    """[n][10] = La Lb Lc Ld nca ncb ncc ncd npp_ab npp_cd"""
    rows = [np.column_stack([L4, ncart(L4), np.full((len(L4), 2), (dab, dcd))]) for dab in depths for dcd in depths]
    return np.concatenate(rows)


def consecutive(q, order, sizes, end="lds_doubles"):
    """the regions in declaration order: each starts where the previous one ended, the last ends at `end`; returns their extents"""
    ext = {}
    assert np.all(q[order[0]] == 0)
    for a, b in zip(order, order[1:] + [end]):
        ext[a] = q[b] - q[a]
        assert np.all(ext[a] >= sizes[a]), a
    return ext


def test_constants():
    assert (THREADS, BLK, CSR, LDS_MAX, pt.const("TEAM_LMAX")) == (256, 1024, 2 * 144 + (2 * 144 + 32) // 2, 160 * 1024 - 256, 6)


def test_multi_kernel_regions():
    c = q_cases((1,))
    c = c[np.prod(c[:, 4:8], axis=1) <= 128]                       # what launch_class sends to eri_multi_kernel
    La, Lb, Lc, Ld, nca, ncb, ncc, ncd = c[:, :8].T
    q = pt.eri_carve("multi", c)
    L, ncomp = La + Lb + Lc + Ld, nca * ncb * ncc * ncd
    tsize, G, kc = (L + 1) * (L + 2) // 2, q["G"], ncc + ncd
    ncp = 2 ** np.ceil(np.log2(ncomp)).astype(np.int64)
    assert np.all(q["ncp"] == ncp) and np.all(G == np.maximum(1, np.minimum(THREADS // ncp, THREADS // (L + 1))))
    assert np.all(G * ncp <= THREADS) and np.all(G * (L + 1) <= THREADS)          # one lane per component, one per (sub-quartet, Boys order)
    assert np.all(q["PB"] == G) and np.all(q["stride"] == G | 1)
    assert np.all(q["offRed"] == q["offEab"])                                      # the documented alias
    need = {"offR": (G | 1) * tsize, "offPref": G, "offPQ": G, "offEab": 2 * nE(La, Lb), "offEcd": G * 2 * nE(Lc, Ld), "offScale": 42 + kc * G,
            "offLmn": (42 + kc * G + G + 1) // 2, "offBlk": G * ncomp, "offCsr": CSR}
    consecutive(q, ["offR", "offPref", "offPQ", "offEab", "offEcd", "offScale", "offLmn", "offBlk", "offCsr"], need)
    assert np.all(q["lds_doubles"] * 8 <= LDS_MAX)


def test_fact_kernel_regions():
    c = q_cases((1,))
    La, Lb, Lc, Ld, nca, ncb, ncc, ncd = c[:, :8].T
    q = pt.eri_carve("fact", c, tupG=1234, tupXZ=5678)
    assert np.all(q["tupG_off"] == 1234) and np.all(q["tupXZ_off"] == 5678)
    L = La + Lb + Lc + Ld
    tsize, nM, nT = (L + 1) * (L + 2) // 2, L // 2 + 1, (La + 1) * (Lb + 1) * (Lc + 1) * (Ld + 1)
    nG = (Lc + 1) * (Ld + 1) * (La + Lb + 1) * nM
    assert np.all(q["offG"] == q["offBlk"])                                        # the ket half of the z tables lives in the block buffer
    over_dead = q["offScale"] >= CSR                                               # R, prefactors, E tables: dead once X and Z are built
    assert np.all(q["offCsr"][over_dead] == 0) and np.all(q["offCsr"][~over_dead] > 0) and over_dead.any() and (~over_dead).any()
    need = {"offR": tsize, "offPref": 1, "offPQ": 1, "offEab": 2 * nE(La, Lb), "offEcd": 2 * nE(Lc, Ld), "offScale": 84, "offLmn": 42,
            "offRed": 2 * nT * nM, "offBlk": np.maximum(BLK, nG), "offTab": 2 * (nca * ncb + ncc * ncd), "offCsr": CSR}
    order = ["offR", "offPref", "offPQ", "offEab", "offEcd", "offScale", "offLmn", "offRed", "offBlk", "offTab"]
    own = {k: v[~over_dead] for k, v in q.items()}
    consecutive(own, order + ["offCsr"], {k: (v[~over_dead] if isinstance(v, np.ndarray) else v) for k, v in need.items()})
    consecutive({k: v[over_dead] for k, v in q.items()}, order, {k: (v[over_dead] if isinstance(v, np.ndarray) else v) for k, v in need.items()})
    eligible = nT * 2 * nM <= 7000                                                 # what launch_class sends to eri_fact_kernel
    assert np.all(q["lds_doubles"][eligible] * 8 <= LDS_MAX)


def test_class_kernel_regions():
    c = q_cases(DEPTHS)
    La, Lb, Lc, Ld = c[:, :4].T
    dab, dcd = c[:, 8], c[:, 9]
    q = pt.eri_carve("class", c)
    L = La + Lb + Lc + Ld
    tsize = (L + 1) * (L + 2) // 2
    PB = np.maximum(1, np.minimum(np.minimum(3584 // tsize - 1, THREADS), dab * dcd))
    assert np.all(q["PB"] == PB) and np.all(q["stride"] == PB | 1) and np.all(q["G"] == 1)
    needE = dab * 2 * nE(La, Lb) + dcd * 2 * nE(Lc, Ld)
    stage = needE <= 3072
    assert np.all((q["stage"] == 1) == stage) and stage.any() and (~stage).any()
    need = {"offR": (PB | 1) * tsize, "offPref": PB, "offPQ": PB, "offRed": THREADS, "offEab": np.where(stage, dab * 2 * nE(La, Lb), 0),
            "offEcd": np.where(stage, dcd * 2 * nE(Lc, Ld), 0), "offScale": 84, "offLmn": 42, "offBlk": BLK, "offCsr": CSR}
    consecutive(q, ["offR", "offPref", "offPQ", "offRed", "offEab", "offEcd", "offScale", "offLmn", "offBlk", "offCsr"], need)
    assert np.all(q["lds_doubles"] * 8 <= LDS_MAX)
    assert np.all(ncart(c[:, 2]) * ncart(c[:, 3]) <= BLK)                          # a (cc, cd) sub-block fits the block buffer


def test_component_lane_kernel_regions():
    q = pt.eri_carve("component_lane", q_cases((1,))[:1])
    # launch-wide capacities: the kernel sizes its batches from offPref - offR and stages E tables that fit offEcd - offEab / offScale - offEcd
    need = {"offR": 2 * ncart(20), "offPref": THREADS, "offPQ": THREADS, "offRed": THREADS, "offEab": 1, "offEcd": 1, "offScale": 84, "offLmn": 42}
    ext = consecutive(q, ["offR", "offPref", "offPQ", "offRed", "offEab", "offEcd", "offScale", "offLmn"], need)
    assert (ext["offR"][0], ext["offEab"][0], ext["offEcd"][0]) == (2048, 1024, 1024)
    assert q["offBlk"][0] == q["lds_doubles"][0] and q["G"][0] == 1 and q["lds_doubles"][0] * 8 <= LDS_MAX


# ---- eri_cfact_kernel -----------------------------------------------------------------------------------------------------------------
def group_stats_of(tag):
    """the GroupStat of each of the 14 pair groups of a basis set, restated: (maxLp, maxT, maxLp1, maxE, maxcomp, maxnpp)"""
    shells = es.system(tag)[1]
    pairs = [[] for _ in range(14)]
    for A, a in enumerate(shells):
        for b in shells[:A + 1]:
            lp, npp = a.L + b.L, len(a.exps) * len(b.exps)
            g = 2 * (0 if lp <= 1 else 1 if lp <= 3 else 2 if lp <= 5 else 3 if lp <= 7 else min(lp - 4, 6)) + (1 if npp > 1 else 0)
            assert g == 2 * pt.eri_lp_group(lp) + (npp > 1)
            pairs[g].append((a.L, b.L, npp, nE(a.L, b.L), ncart(a.L) * ncart(b.L)))
    stats = []
    for p in pairs:
        p = np.array(p, dtype=np.int64).reshape(-1, 5)
        want = (0, 1, 1, 0, 1, 1) if not len(p) else (int((p[:, 0] + p[:, 1]).max()), int(((p[:, 0] + 1) * (p[:, 1] + 1)).max()),
                                                      int((p[:, 0] + p[:, 1]).max()) + 1, int((p[:, 2] * 2 * p[:, 3]).max()), int(p[:, 4].max()), int(p[:, 2].max()))
        assert pt.eri_group_stat(p) == want
        stats.append(want)
    return stats


def cfact_cases():
    """[n][21]: every (bra group, ket group) of every system, and every pair of single-(La, Lb, depth) groups; families on and off"""
    rows = []
    for tag in SYSTEM_TAGS:
        gs = group_stats_of(tag)
        for gb in range(14):
            for gk in range(14):
                for km in (0, 9):
                    rows.append(gs[gb] + gs[gk] + (gb & 1, gk & 1, 24, 768, 1024, km, 1, -1, 700))
    single = [(la + lb, (la + 1) * (lb + 1), la + lb + 1, d * 2 * nE(la, lb), ncart(la) * ncart(lb), d) for la in range(6) for lb in range(6) for d in DEPTHS]
    for sb in single:
        for sk in single:
            rows.append(sb + sk + (int(sb[5] > 1), int(sk[5] > 1), 24, 768, 1024, 9, 0, 6, 700))
    return np.array(rows, dtype=np.int64)


def test_cfact_regions():
    c = cfact_cases()
    q = pt.eri_cfact(c)
    (bLp, bT, bLp1, bE, _, bnpp), (kLp, kT, _, kE, _, knpp) = c[:, 0:6].T, c[:, 6:12].T
    bra_c, ket_c, k_nbt, k_xz, k_e, km, packed, tl, tpq = c[:, 12:].T
    Lmax = bLp + kLp
    nM, tsize = Lmax // 2 + 1, (Lmax + 1) * (Lmax + 2) // 2
    xz, gsz = bT * kT * nM, kT * bLp1 * nM
    deep = (bnpp > 1) | (knpp > 1)
    fit, gtab = q["fit"] == 1, q["gtab"] == 1
    lds = ~gtab
    # the largest tuple of the two groups fits every table; the staged Hermite tables are capped by the knob
    assert np.all(q["capR"] >= 2 * tsize) and np.all(q["capG"] >= gsz) and np.all(q["capXZ"] >= xz)
    assert np.all(q["capEab"] == np.minimum(bE, k_e)) and np.all(q["capEcd"] == np.minimum(kE, k_e))
    assert np.all(q["capKm"] == km * (np.where(ket_c == 1, knpp, 0) + np.where(bra_c == 1, bnpp, 0)))
    assert np.all(q["tri"] == packed) and np.all(q["team_lmax"] == tl) and np.all(q["team_pqmax"] == tpq)
    assert np.all(q["dbg_npq_lo"] == 0) and np.all(q["dbg_npq_hi"] == 0x7fffffff)
    need = {"offR": q["capR"], "offPref": THREADS, "offPQ": THREADS, "offPP": THREADS, "offG": q["capG"], "offX": q["capXZ"], "offZ": q["capXZ"],
            "offTupG": (gsz + 3) // 4, "offTupXZ": (xz + 3) // 4, "offEab": q["capEab"], "offEcd": q["capEcd"], "offRed": THREADS, "offKm": q["capKm"]}
    order = ["offR", "offPref", "offPQ", "offPP", "offG", "offX", "offZ", "offTupG", "offTupXZ", "offEab", "offEcd", "offRed", "offKm"]
    pick = lambda m: ({k: v[m] for k, v in q.items()}, {k: (v[m] if isinstance(v, np.ndarray) else v) for k, v in need.items()})
    consecutive(*[pick(lds)[0], order, pick(lds)[1]])
    assert np.all(fit[lds] == (q["lds_doubles"][lds] * 8 <= LDS_MAX)) and fit[lds].any() and (~fit[lds]).any()
    assert np.all(q["gtab_doubles"][lds] == 0)
    # global-table plans: only for uncontracted group pairs whose LDS plan does not fit; G, X, Z relative to the workgroup's global block
    assert gtab.any() and not np.any(deep[gtab]) and np.all(fit[gtab])
    g, n = pick(gtab)
    consecutive(g, [o for o in order if o not in ("offG", "offX", "offZ")], n)
    assert np.all(g["lds_doubles"] * 8 <= LDS_MAX)
    assert np.all(g["offG"] == 0) and np.all(g["offX"] == gsz[gtab]) and np.all(g["offZ"] == (gsz + xz)[gtab])
    assert np.all(g["capG"] == gsz[gtab]) and np.all(g["capXZ"] == xz[gtab]) and np.all(g["gtab_doubles"] == (gsz + 2 * xz)[gtab])
    # ... whose LDS plan (restated: the thirteen regions) would not have fitted
    nbt = np.where(deep, np.minimum(THREADS // (Lmax + 1), k_nbt), 1)
    capR = np.maximum(2 * tsize, np.minimum((nbt + 1) * tsize, 2 * k_xz * 2 // 3))
    capG, capXZ = np.maximum(gsz, np.minimum(nbt * gsz, k_xz * 2 // 3)), np.maximum(xz, np.minimum(nbt * xz, k_xz))
    full = capR + 4 * THREADS + capG + 2 * capXZ + (gsz + 3) // 4 + (xz + 3) // 4 + np.minimum(bE, k_e) + np.minimum(kE, k_e) + q["capKm"]
    assert np.all(full[gtab] * 8 > LDS_MAX) and np.all(full[lds] == q["lds_doubles"][lds])
    assert np.all(capR[lds] == q["capR"][lds]) and np.all(capG[lds] == q["capG"][lds]) and np.all(capXZ[lds] == q["capXZ"][lds])
    assert np.all((~fit) == ((full * 8 > LDS_MAX) & ~gtab))


def test_lrec_batch_capacity_and_index_words():
    caps_all = pt.eri_cfact(cfact_cases()[-400:])
    caps = np.column_stack([caps_all["capR"], caps_all["capG"], caps_all["capXZ"]])[::7]
    for La, Lb, Lc, Ld in L4[::5]:
        r0, words = pt.eri_lrec((La, Lb, Lc, Ld))
        L = La + Lb + Lc + Ld
        nM, nT = L // 2 + 1, (La + 1) * (Lb + 1) * (Lc + 1) * (Ld + 1)
        assert (r0["L"], r0["nM"], r0["tsize"], r0["nT"], r0["xz"], r0["gsz"]) == (L, nM, (L + 1) * (L + 2) // 2, nT, nT * nM, (Lc + 1) * (Ld + 1) * (La + Lb + 1) * nM)
        for lg, n in ((r0["lgG"], r0["gsz"]), (r0["lgX"], r0["xz"])):
            assert 2 ** lg >= min(n, THREADS) and (lg == 0 or 2 ** (lg - 1) < min(n, THREADS))
        assert r0["nb_cap"] == max(1, THREADS // (L + 1)) and r0["pad"] == 0
        r, _ = pt.eri_lrec((La, Lb, Lc, Ld), caps)
        applies = (caps[:, 0] >= 2 * r["tsize"]) & (caps[:, 1] >= r["gsz"]) & (caps[:, 2] >= r["xz"])
        assert 1 <= r["nb_cap"] <= r0["nb_cap"]
        for capR, capG, capXZ in caps[applies]:
            assert (r["nb_cap"] + 1) * r["tsize"] <= capR and r["nb_cap"] * r["gsz"] <= capG and r["nb_cap"] * r["xz"] <= capXZ
        if applies.any():
            a = caps[applies]
            assert r["nb_cap"] == max(1, min(r0["nb_cap"], int((a[:, 0] // r["tsize"] - 1).min()), int((a[:, 1] // r["gsz"]).min()), int((a[:, 2] // r["xz"]).min())))
        # the words decode back to the loop indices of their entry
        e = np.arange(r["gsz"])
        w = words[:r["gsz"]].astype(np.int64)
        n, v, d, cc = e % nM, e // nM % (La + Lb + 1), e // (nM * (La + Lb + 1)) % (Ld + 1), e // (nM * (La + Lb + 1) * (Ld + 1))
        assert np.all(w & 15 == n) and np.all((w >> 4) & 15 == v) and np.all((w >> 8) & 7 == d) and np.all(w >> 11 == cc)
        e = np.arange(r["xz"])
        w = words[r["gsz"]:].astype(np.int64)
        m, d, cc, b2, a2 = e % nM, e // nM % (Ld + 1), e // (nM * (Ld + 1)) % (Lc + 1), e // (nM * (Ld + 1) * (Lc + 1)) % (Lb + 1), e // (nM * (Ld + 1) * (Lc + 1) * (Lb + 1))
        assert np.all(w & 15 == m) and np.all((w >> 4) & 7 == a2) and np.all((w >> 7) & 7 == b2) and np.all((w >> 10) & 7 == cc) and np.all(w >> 13 == d)


# ---- team kernels -------------------------------------------------------------------------------------------------------------------
def parity_counts(L, spherical):
    """functions of a shell by x/y parity class (lx & 1 | (ly & 1) << 1): Cartesian components, output functions"""
    comp = np.zeros(4, dtype=np.int64)
    for lx in range(L + 1):
        for ly in range(L + 1 - lx):
            comp[(lx & 1) | ((ly & 1) << 1)] += 1
    if not spherical:
        return comp, comp.copy()
    out = np.zeros(4, dtype=np.int64)                    # real solid harmonics: cos(m phi) -> (m & 1, 0), sin(m phi) -> ((m + 1) & 1, 1), z parity free
    for m in range(-L, L + 1):
        out[((abs(m) + 1) & 1) | 2 if m < 0 else (m & 1)] += 1
    return comp, out


def pair_classes(ca, cb):
    return np.array([sum(ca[x] * cb[x ^ c] for x in range(4)) for c in range(4)], dtype=np.int64)


def team_cases(spherical, foff):
    rows = []
    for La, Lb, Lc, Ld in L4:
        if La + Lb > 6 or Lc + Ld > 6:
            continue
        (ca, _), (cb, _), (cc, oc), (cd, od) = (parity_counts(L, spherical) for L in (La, Lb, Lc, Ld))
        pA, pK, pS = pair_classes(ca, cb), pair_classes(cc, cd), pair_classes(oc, od)
        nab, ncd, nkap = int(pA.sum()), int(pK.sum()), int(pS.sum())
        assert (nab, ncd) == (ncart(La) * ncart(Lb), ncart(Lc) * ncart(Ld))
        nnzT = ncd if not spherical else int(sum(pS[c] * max(1, pK[c] // 2) for c in range(4)))   # (any count: the plan takes it as a size)
        nnzc, maxblk, maxK, nout = int((pA * pK).sum()), int((pA * pK).max()), int(pK.max()), int((pA * pS).sum())
        rows.append((La, Lb, Lc, Ld, nab, ncd, nkap, nnzT, nnzc, nout, foff if nnzc <= 2048 else -1, max(1, maxblk), max(1, maxK), nnzc, nE(La, Lb), nE(Lc, Ld)))
    return np.array(rows, dtype=np.int64)


def even(x):
    return (x + 1) // 2 * 2


@pytest.mark.parametrize("foff", [-1, 40])
@pytest.mark.parametrize("spherical", [True, False])
def test_team_kernel_regions(spherical, foff):
    c = team_cases(spherical, foff)
    La, Lb, Lc, Ld, nab, ncd, nkap, nnzT, nacc, nout, fo, maxblk, maxK, nnzc, nEab, nEcd = c.T
    t = pt.eri_team(True, c)
    LAB, L = La + Lb, La + Lb + Lc + Ld
    NM, nT, nTcd = L // 2 + 1, (La + 1) * (Lb + 1) * (Lc + 1) * (Ld + 1), (Lc + 1) * (Ld + 1)
    need = {"oE12": 2 * nEab, "oOffA": 2 * nab, "oScA": nab, "oOffK": 2 * ncd, "oTp": (nkap + 2) // 2, "oTk": (nnzT + 1) // 2, "oTc": nnzT, "oRowOff": nab}
    consecutive(t, ["oE12", "oOffA", "oScA", "oOffK", "oTp", "oTk", "oTc", "oRowOff"], need, end="oCompW")
    assert np.all(t["oOutW"] == t["oCompW"] + even(nnzc) // 2) and np.all(t["nflat"] == even(nnzc) + 2 * nout) and np.all(t["flat_off"] == np.maximum(0, fo))
    scr1 = 2 * nEcd + (L + 1) * (L + 2) + nTcd * (LAB + 1) * NM               # ket Hermite tables, R rows, G of a team
    for tm, vmax in ((16, 96), (64, 512), (256, 2048)):
        flat = (fo >= 0) & (nnzc <= vmax)
        assert np.all((t[f"flat_{tm}"] == 1) == flat)
        assert np.all(t[f"shared_doubles_{tm}"] == t["oCompW"] + np.where(flat, even((t["nflat"] + 1) // 2), 0))
        assert np.all(t[f"vcap_{tm}"] >= np.where(flat, np.maximum(scr1, nnzc), np.maximum(scr1, np.maximum(maxK, np.minimum(maxblk, vmax)))))
        assert np.all(t[f"team_doubles_{tm}"] >= 2 * nT * (NM | 1) + t[f"vcap_{tm}"] + (nkap + 1) // 2)
        assert np.all(t[f"bytes_{tm}"] == 8 * (t[f"shared_doubles_{tm}"] + (256 // tm) * t[f"team_doubles_{tm}"]))


@pytest.mark.parametrize("spherical", [True, False])
def test_teamc_kernel_regions(spherical):
    c = team_cases(spherical, -1)
    La, Lb, Lc, Ld, nab, ncd, nkap, nnzT, nacc, nout, fo, maxblk, maxK, nnzc, nEab, nEcd = c.T
    t = pt.eri_team(False, c)
    LAB, L = La + Lb, La + Lb + Lc + Ld
    NM, nT, nTcd = L // 2 + 1, (La + 1) * (Lb + 1) * (Lc + 1) * (Ld + 1), (Lc + 1) * (Ld + 1)
    assert np.all(t["oE12"] == 0) and np.all(t["oOffA"] == 0) and np.all(t["oRowOff"] == 0)   # the Hermite tables live in the team's scratch
    t["end"] = t["shared_doubles_64"]
    need = {"oOffA": 2 * nab, "oScA": nab, "oOffK": 2 * ncd, "oTp": (nkap + 2) // 2, "oTk": (nnzT + 1) // 2, "oTc": nnzT}
    consecutive(t, ["oOffA", "oScA", "oOffK", "oTp", "oTk", "oTc"], need, end="end")
    for tm in (16, 64, 256):
        assert np.all(t[f"vcap_{tm}"] >= 2 * nEab + 2 * nEcd + (L + 1) * (L + 2) + nTcd * (LAB + 1) * NM) and np.all(t[f"flat_{tm}"] == 0)
        assert np.all(t[f"team_doubles_{tm}"] >= 2 * nT * (NM | 1) + t[f"vcap_{tm}"] + nacc + (nkap + 1) // 2)
        assert np.all(t[f"bytes_{tm}"] == 8 * (t["end"] + (256 // tm) * t[f"team_doubles_{tm}"]))


KB = 1024
PER_CLASS, TEAMC = dict(soft64=76 * KB, t16_nnz=96, force=0), dict(soft64=52 * KB, t16_nnz=96, force=0)
# written out by hand from the cascades of launch_class (76 KB from the knob) and teamc_class (52 KB): avail, bytes (16, 64, 256), nT, nnzc -> team
HAND_CASES = [
    ("a 16-lane class", PER_CLASS, (1, 1, 0), (9 * KB, 12 * KB, 0), 4, 5, 16),
    ("a 16-lane class, teamc", TEAMC, (1, 1, 0), (9 * KB, 12 * KB, 0), 16, 96, 16),
    ("nnz above the 16-lane limit", PER_CLASS, (1, 1, 0), (9 * KB, 12 * KB, 0), 16, 97, 64),
    ("nT above 16", PER_CLASS, (1, 1, 1), (9 * KB, 40 * KB, 30 * KB), 24, 40, 64),
    ("64 lanes under the soft limit", PER_CLASS, (0, 1, 1), (0, 76 * KB, 50 * KB), 144, 900, 64),
    ("60 KB: under 76, above teamc's 52 -> 256", TEAMC, (0, 1, 1), (0, 60 * KB, 50 * KB), 144, 900, 256),
    ("60 KB per class stays 64", PER_CLASS, (0, 1, 1), (0, 60 * KB, 50 * KB), 144, 900, 64),
    ("pushed to 256", PER_CLASS, (0, 1, 1), (0, 76 * KB + 8, 120 * KB), 256, 3000, 256),
    ("256 at the hard limit", PER_CLASS, (0, 1, 1), (0, 100 * KB, 160 * KB - 256), 256, 3000, 256),
    ("back to 64 under the hard limit: 256 too large", PER_CLASS, (0, 1, 1), (0, 100 * KB, 160 * KB - 248), 256, 3000, 64),
    ("back to 64 under the hard limit: 256 not instantiated", TEAMC, (0, 1, 0), (0, 100 * KB, 20 * KB), 100, 3000, 64),
    ("no team: nothing fits", PER_CLASS, (0, 1, 1), (0, 160 * KB, 161 * KB), 256, 3000, 0),
    ("no team: nothing instantiated", TEAMC, (0, 0, 0), (KB, KB, KB), 4, 4, 0),
    ("forced 256", dict(PER_CLASS, force=256), (1, 1, 1), (9 * KB, 12 * KB, 30 * KB), 4, 5, 256),
    ("forced 64 over a 256 choice", dict(PER_CLASS, force=64), (0, 1, 1), (0, 100 * KB, 120 * KB), 256, 3000, 64),
    ("forced size not instantiated", dict(PER_CLASS, force=256), (1, 1, 0), (9 * KB, 12 * KB, KB), 4, 5, 16),
    ("forced size too large", dict(PER_CLASS, force=256), (1, 1, 1), (9 * KB, 12 * KB, 161 * KB), 4, 5, 16),
    ("forced size that does not exist", dict(PER_CLASS, force=32), (1, 1, 1), (9 * KB, 12 * KB, 30 * KB), 4, 5, 16),
]


@pytest.mark.parametrize("case", HAND_CASES, ids=[c[0] for c in HAND_CASES])
def test_team_choice_by_hand(case):
    _, par, avail, nbytes, nT, nnzc, want = case
    assert pt.eri_choose_team(avail, nbytes, nT, nnzc, **par) == want


def test_team_choice_rules():
    """over the byte counts of every class of the range (both kernels' plans, both sets of parameters, every forced size)"""
    n = 0
    for per_class, par in ((True, PER_CLASS), (False, TEAMC)):
        for spherical in (True, False):
            c = team_cases(spherical, 40 if per_class else -1)
            t = pt.eri_team(per_class, c)
            for k, row in enumerate(c):
                LAB, LCD = row[0] + row[1], row[2] + row[3]
                nT, nnzc = (row[0] + 1) * (row[1] + 1) * (row[2] + 1) * (row[3] + 1), row[13]
                avail = [es.team_size_instantiated(LAB, LCD, tm) for tm in (16, 64, 256)]
                nbytes = [int(t[f"bytes_{tm}"][k]) for tm in (16, 64, 256)]
                free = pt.eri_choose_team(avail, nbytes, nT, nnzc, **par)
                for force in (0, 16, 64, 256) if per_class else (0,):
                    team = pt.eri_choose_team(avail, nbytes, nT, nnzc, **dict(par, force=force))
                    assert team in (0, 16, 64, 256)
                    if team:
                        s = (16, 64, 256).index(team)
                        assert avail[s] and nbytes[s] <= LDS_MAX
                    ok = force and avail[(16, 64, 256).index(force)] and nbytes[(16, 64, 256).index(force)] <= LDS_MAX
                    assert team == (force if ok else free)
                    if team == 16 and not ok:
                        assert nT <= 16 and nnzc <= par["t16_nnz"]
                    n += 1
    assert n > 5000


def test_team_grid():
    # ket groups per workgroup: max(1, min(kpw_max, groups * n_bra / kpw_div)); the grid covers every group
    for n_ket, team, n_bra, div, mx in ((1, 16, 1, 2048, 16), (1000, 16, 50, 2048, 16), (100000, 64, 3000, 2048, 16), (777, 256, 65535, 2048, 16),
                                        (100000, 64, 3000, 1, 1), (12345, 64, 17, 64, 5)):
        NT = 256 // team
        groups = (n_ket + NT - 1) // NT
        kpw = max(1, min(mx, groups * n_bra // div))
        assert pt.eri_team_grid_x(n_ket, team, n_bra, div, mx) == (groups + kpw - 1) // kpw
