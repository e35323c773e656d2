// tf_eri_plan.h -- the LDS carve-outs of every ERI kernel family, the team-size choice and the per-tuple records of eri_cfact_kernel,
// as pure functions that fill the launch records of tf_eri_types.h from integers.  No HIP, no environment, no context: the launch
// functions of tf_eri_host.hip.h pass the knob values in; tests/packed_model compiles this header for the CPU and
// tests/test_eri_plan.py checks every region against the formulas of the kernel headers.  DESIGN.md section 3.1.
#pragma once
#include <algorithm>
#include <cstddef>
#include "tf_eri_types.h"

namespace tfe {
using tfk::CFCaps; using tfk::LRec; using tfk::QClass; using tfk::TClass;

// what a workgroup may ask for: the 160 KB of a CU less what the runtime keeps
static const size_t ERI_LDS_MAX_BYTES = 160 * 1024 - 256;
static inline size_t lds_bytes(int doubles) { return (size_t)doubles * sizeof(double); }

// ---- per-class mode: eri_multi_kernel, eri_fact_kernel, eri_class_kernel.  q holds the class (angular momenta, component counts,
// depths, table sizes); the carve functions add the batch shape and the offsets.

// several uncontracted shell quartets per workgroup
static inline void carve_multi(QClass &q)
{
    int ncp = 1;
    while (ncp < q.ncomp) ncp <<= 1;
    q.ncp = ncp;
    q.G = std::max(1, std::min(TF_ERI_THREADS / ncp, TF_ERI_THREADS / (q.L + 1)));
    q.PB = q.G; q.stride = q.G | 1;
    const int kc = q.ncc + q.ncd;
    int o = 0;
    q.offR = o; o += q.stride * q.tsize;
    q.offPref = o; o += q.G;
    q.offPQ = o; o += q.G;
    q.offRed = o;
    q.offEab = o; o += 2 * q.nEab;
    q.offEcd = o; o += q.G * 2 * q.nEcd;
    q.offScale = o; o += 42 + kc * q.G;
    q.offLmn = o; o += (42 + kc * q.G + q.G + 1) / 2;
    q.offBlk = o; o += q.G * q.ncomp;
    q.offCsr = o; o += TF_CSR_DOUBLES;
    q.lds_doubles = o;
}

// uncontracted, many components: per-axis factor tables in LDS (tupG_off / tupXZ_off: the LRec of the class)
static inline void carve_fact(QClass &q, int tupG_off, int tupXZ_off)
{
    const int nT = (q.La + 1) * (q.Lb + 1) * (q.Lc + 1) * (q.Ld + 1), nM = q.L / 2 + 1;
    q.PB = 1; q.stride = 1; q.G = 1; q.ncp = 0;
    q.tupG_off = tupG_off; q.tupXZ_off = tupXZ_off;
    int o = 0;
    q.offR = o; o += q.tsize;
    q.offPref = o; o += 2;
    q.offPQ = o; o += 2;
    q.offEab = o; o += 2 * q.nEab;
    q.offEcd = o; o += 2 * q.nEcd;
    const int tables_end = o;                            // R, prefactors and E tables: dead once X and Z are built
    q.offScale = o; o += 84;
    q.offLmn = o; o += 42;
    q.offRed = o; o += 2 * nT * nM;                      // X and Z tables
    const int nG = (q.Lc + 1) * (q.Ld + 1) * (q.La + q.Lb + 1) * nM;
    q.offBlk = o; o += std::max((int)TF_BLK_DOUBLES, nG);   // the ket half of the z tables lives here until the components start
    q.offG = q.offBlk;
    q.offTab = o; o += 2 * (q.nca * q.ncb + q.ncc * q.ncd) + 2;
    if (tables_end >= TF_CSR_DOUBLES) q.offCsr = 0;      // staged over the dead tables (after the X/Z barrier)
    else { q.offCsr = o; o += TF_CSR_DOUBLES; }
    q.lds_doubles = o;
}

// one shell quartet per workgroup, primitive quartets in LDS batches; returns whether the E tables are staged
static inline bool carve_class(QClass &q)
{
    const int RB = 3584, EB = 3072;                     // LDS doubles for R tables / staged E tables
    int PB = RB / q.tsize - 1;
    PB = std::max(1, std::min(std::min(PB, TF_ERI_THREADS), q.npq));
    q.PB = PB; q.stride = PB | 1; q.G = 1; q.ncp = 0;
    const int needE = q.npp_ab * 2 * q.nEab + q.npp_cd * 2 * q.nEcd;
    const bool stage = needE <= EB;
    int o = 0;
    q.offR = o; o += q.stride * q.tsize;
    q.offPref = o; o += TF_ERI_THREADS;
    q.offPQ = o; o += TF_ERI_THREADS;
    q.offRed = o; o += TF_ERI_THREADS;
    q.offEab = o; o += stage ? q.npp_ab * 2 * q.nEab : 0;
    q.offEcd = o; o += stage ? q.npp_cd * 2 * q.nEcd : 0;
    q.offScale = o; o += 84;
    q.offLmn = o; o += 42;
    q.offBlk = o; o += TF_BLK_DOUBLES;
    q.offCsr = o; o += TF_CSR_DOUBLES;
    q.lds_doubles = o;
    return stage;
}

// ---- small-problem mode: the component-per-lane kernel (eri_class_kernel<true, true>, unfused) and eri_cfact_kernel

static inline void carve_component_lane(QClass &q)
{
    const int RB = 2048, EBa = 1024, EBc = 1024;       // (doubling the E capacities halves the occupancy: Ar2 build 0.084 -> 0.18 s)
    int o = 0;
    q.offR = o; o += RB;
    q.offPref = o; o += TF_ERI_THREADS;
    q.offPQ = o; o += TF_ERI_THREADS;
    q.offRed = o; o += TF_ERI_THREADS;
    q.offEab = o; o += EBa;
    q.offEcd = o; o += EBc;
    q.offScale = o; o += 84;
    q.offLmn = o; o += 42;
    q.lds_doubles = o;
    q.offBlk = o;                                            // unused (unfused)
    q.G = 1;
}

// groups of shell pairs: by La + Lb (0-1, 2-3, 4-5, 6-7, 8, 9, 10: the table sizes grow with the fourth power of L, and only the
// very top -- (hh|hh), (hh|gh), ... -- exceeds LDS and falls back to the component-per-lane kernel) and by contracted / uncontracted
static inline int lp_group(int lp) { return lp <= 1 ? 0 : (lp <= 3 ? 1 : (lp <= 5 ? 2 : (lp <= 7 ? 3 : std::min(lp - 4, 6)))); }

// the largest angular momenta / contraction depths of a group: one call per shell pair (ncomp: component pairs of the pair)
struct GroupStat { int maxLp = 0, maxT = 1, maxLp1 = 1, maxE = 0, maxcomp = 1, maxnpp = 1; };
static inline void group_stat(GroupStat &g, int La, int Lb, int npp, int nE, int ncomp)
{
    g.maxLp = std::max(g.maxLp, La + Lb);
    g.maxT = std::max(g.maxT, (La + 1) * (Lb + 1));
    g.maxE = std::max(g.maxE, npp * 2 * nE);
    g.maxcomp = std::max(g.maxcomp, ncomp);
    g.maxnpp = std::max(g.maxnpp, npp);
    g.maxLp1 = g.maxLp + 1;
}

// batch size aimed at and LDS doubles for the X / Z tables and the staged Hermite tables (tuning knobs; smaller carve-outs
// mean more workgroups per CU: Ar2/cc-pVQZ ERI kernels 21.1 ms with 48 / 1536 / 1536, 18.3 ms with 24 / 768 / 1024)
struct CFKnobs { int nbt = 24, xz = 768, e = 1024; };
struct CFPlan { CFCaps caps; bool fit, gtab; };

// LDS carve-out of the launch (bra group, ket group), from the largest angular momenta / contraction depths of the groups.
// km_members: weights staged per primitive pair of a contracted side (0: families off); the debug window is the caller's.
static inline CFPlan carve_cfact(const GroupStat &sb, const GroupStat &sk, bool bra_contracted, bool ket_contracted, const CFKnobs &k,
                                 int km_members, bool packed, int team_lmax, int team_pqmax)
{
    const int Lmax = sb.maxLp + sk.maxLp, nM = Lmax / 2 + 1, tsize = (Lmax + 1) * (Lmax + 2) / 2;
    const int xz = sb.maxT * sk.maxT * nM, gsz = sk.maxT * sb.maxLp1 * nM;
    const bool deep = sb.maxnpp > 1 || sk.maxnpp > 1;
    const int nbt = deep ? std::min(TF_ERI_THREADS / (Lmax + 1), k.nbt) : 1;       // primitive quartets per batch aimed at
    CFCaps c{};
    int o = 0;
    c.offR = o; c.capR = std::max(2 * tsize, std::min((nbt + 1) * tsize, 2 * k.xz * 2 / 3)); o += c.capR;
    c.offPref = o; o += TF_ERI_THREADS;
    c.offPQ = o; o += TF_ERI_THREADS;
    c.offPP = o; o += TF_ERI_THREADS;
    c.offG = o; c.capG = std::max(gsz, std::min(nbt * gsz, k.xz * 2 / 3)); o += c.capG;
    c.capXZ = std::max(xz, std::min(nbt * xz, k.xz));
    c.offX = o; o += c.capXZ;
    c.offZ = o; o += c.capXZ;
    c.offTupG = o; o += (gsz + 3) / 4;
    c.offTupXZ = o; o += (xz + 3) / 4;
    c.offEab = o; c.capEab = std::min(sb.maxE, k.e); o += c.capEab;
    c.offEcd = o; c.capEcd = std::min(sk.maxE, k.e); o += c.capEcd;
    c.offRed = o; o += TF_ERI_THREADS;
    c.offKm = o; c.capKm = km_members * ((ket_contracted ? sk.maxnpp : 0) + (bra_contracted ? sb.maxnpp : 0)); o += c.capKm;
    c.lds_doubles = o;
    c.tri = packed ? 1 : 0;
    c.dbg_npq_lo = 0; c.dbg_npq_hi = 0x7fffffff;
    c.team_lmax = team_lmax; c.team_pqmax = team_pqmax;
    CFPlan P{c, lds_bytes(o) <= ERI_LDS_MAX_BYTES, false};
    if (!P.fit && !deep) {
        // (hh|hh)-sized tables: G, X and Z of a workgroup go to global memory, everything else stays in LDS
        CFCaps d = c;
        int q = 0;
        d.offR = q; q += d.capR;
        d.offPref = q; q += TF_ERI_THREADS;
        d.offPQ = q; q += TF_ERI_THREADS;
        d.offPP = q; q += TF_ERI_THREADS;
        d.offTupG = q; q += (gsz + 3) / 4;
        d.offTupXZ = q; q += (xz + 3) / 4;
        d.offEab = q; q += d.capEab;
        d.offEcd = q; q += d.capEcd;
        d.offRed = q; q += TF_ERI_THREADS;
        d.offKm = q; q += d.capKm;
        d.lds_doubles = q;
        d.capG = gsz; d.capXZ = xz;
        d.offG = 0; d.offX = gsz; d.offZ = gsz + xz;
        d.gtab_doubles = gsz + 2 * xz;
        if (lds_bytes(q) <= ERI_LDS_MAX_BYTES) P = CFPlan{d, true, true};
    }
    return P;
}

// per (La, Lb | Lc, Ld): table sizes of eri_cfact_kernel; nb_cap starts at what the workgroup's lanes allow
static inline LRec lrec_sizes(int La, int Lb, int Lc, int Ld)
{
    LRec r{};
    r.L = La + Lb + Lc + Ld; r.nM = r.L / 2 + 1; r.tsize = (r.L + 1) * (r.L + 2) / 2;
    r.nT = (La + 1) * (Lb + 1) * (Lc + 1) * (Ld + 1); r.xz = r.nT * r.nM;
    r.gsz = (Lc + 1) * (Ld + 1) * (La + Lb + 1) * r.nM;
    r.lgG = 0; while ((1 << r.lgG) < r.gsz && (1 << r.lgG) < TF_ERI_THREADS) ++r.lgG;
    r.lgX = 0; while ((1 << r.lgX) < r.xz && (1 << r.lgX) < TF_ERI_THREADS) ++r.lgX;
    r.nb_cap = std::max(TF_ERI_THREADS / (r.L + 1), 1);
    return r;
}
// whether a launch with these caps can hold a quartet of the tuple at all
static inline bool lrec_applies(const LRec &r, const CFCaps &c) { return !(c.capR < 2 * r.tsize || c.capG < r.gsz || c.capXZ < r.xz); }
// batch capacity: the smallest over the launches (contracted bra and / or ket group) this tuple can occur in
static inline void lrec_limit(LRec &r, const CFCaps &c)
{
    if (!lrec_applies(r, c)) return;                     // (no such quartet in that launch)
    int nb = std::min(r.nb_cap, c.capR / r.tsize - 1);
    nb = std::min(nb, std::min(c.capG / r.gsz, c.capXZ / r.xz));
    r.nb_cap = std::max(nb, 1);
}
// entry e of the G table = ((cc (Ld + 1) + d) Lab1 + v) nM + n, of the X / Z tables = (((a2 (Lb + 1) + b2) (Lc + 1) + cc) (Ld + 1) + d) nM + m
// (nested loops in that order: a cc-pVQZ basis has 625 tuples and 6e5 entries -- with a division chain per entry this was
// 2 ms of every tensor build).  tp: r.gsz + r.xz words, the G words first.
static inline void lrec_words(const LRec &r, int La, int Lb, int Lc, int Ld, unsigned short *tp)
{
    const int Lab1 = La + Lb + 1;
    for (int cc = 0; cc <= Lc; ++cc)
        for (int d = 0; d <= Ld; ++d)
            for (int v = 0; v < Lab1; ++v)
                for (int n = 0; n < r.nM; ++n) *tp++ = (unsigned short)(n | (v << 4) | (d << 8) | (cc << 11));
    for (int a2 = 0; a2 <= La; ++a2)
        for (int b2 = 0; b2 <= Lb; ++b2)
            for (int cc = 0; cc <= Lc; ++cc)
                for (int d = 0; d <= Ld; ++d)
                    for (int m = 0; m < r.nM; ++m) *tp++ = (unsigned short)(m | (a2 << 4) | (b2 << 7) | (cc << 10) | (d << 13));
}

// ---- team kernels (tf_eri_team.hip.h, tf_eri_teamc.hip.h).  t holds the class-wide part (EriBuild::tclass_common).
static inline int team_even(int x) { return (x + 1) & ~1; }
static inline int team_slot(int team) { return team == 256 ? 2 : (team == 64 ? 1 : 0); }   // index of a team size in the arrays below
static const int TEAM_SIZES[3] = {16, 64, 256};

// The region every team of a workgroup shares.  per_class (eri_team_kernel): the bra Hermite tables in front, the row offsets behind;
// eri_teamc_kernel keeps its Hermite tables in the team's scratch (oE12 = 0).  Returns the end of the region.
static inline int carve_team_shared(TClass &t, bool per_class)
{
    int o = 0;
    t.oE12 = o; o += per_class ? team_even(2 * t.nEab) : 0;
    t.oOffA = o; o += 2 * t.nab;
    t.oScA = o; o += team_even(t.nab);
    t.oOffK = o; o += 2 * t.ncd;
    t.oTp = o; o += team_even((t.nkap + 2) / 2);
    t.oTk = o; o += team_even((t.nnzT + 1) / 2);
    t.oTc = o; o += team_even(t.nnzT);
    if (per_class) { t.oRowOff = o; o += t.nab; }
    t.shared_doubles = o;
    return o;
}

// what a class costs at each team size (index: team_slot)
struct TeamSizes { int vcap[3], team_doubles[3], shared[3]; bool flat[3]; size_t bytes[3]; };

// eri_team_kernel: shared region with the flat lists (foff: the class's position in DBasis::tflat, -1: none) and the three sizes.
// maxblk / maxK / nnzc: largest parity block, most ket component pairs of a parity class, parity-allowed components.
static inline TeamSizes carve_team(TClass &t, int foff, int maxblk, int maxK, int nnzc)
{
    const int LAB = t.La + t.Lb, L = LAB + t.Lc + t.Ld, NM = L / 2 + 1, XS = NM | 1, RSr = L + 2;
    const int shared_noflat = carve_team_shared(t, true);
    const int nacc_pad = team_even(nnzc);
    t.oCompW = shared_noflat; t.oOutW = shared_noflat + nacc_pad / 2; t.flat_off = std::max(0, foff); t.nflat = nacc_pad + 2 * t.nout;
    const int flat_doubles = team_even((t.nflat + 1) / 2);
    const int nG = t.nTcd * (LAB + 1) * NM, scr1 = 2 * t.nEcd + (L + 1) * RSr + nG;
    TeamSizes S{};
    for (int s = 0; s < 3; ++s) {
        const int tm = TEAM_SIZES[s], vmax = tm == 256 ? 2048 : (tm == 64 ? 512 : 96);
        // (a class whose parity-allowed components fit the team's block runs the flat lists: one loop over all components)
        S.flat[s] = foff >= 0 && nnzc <= vmax;
        S.vcap[s] = S.flat[s] ? team_even(std::max(scr1, nnzc)) : team_even(std::max(scr1, std::max(maxK, std::min(maxblk, vmax))));
        S.team_doubles[s] = 2 * t.nT * XS + S.vcap[s] + team_even((t.nkap + 1) / 2);
        S.shared[s] = shared_noflat + (S.flat[s] ? flat_doubles : 0);
        S.bytes[s] = ((size_t)S.shared[s] + (size_t)(256 / tm) * S.team_doubles[s]) * sizeof(double);
    }
    return S;
}
static inline void team_apply(TClass &t, const TeamSizes &S, int team)
{
    const int s = team_slot(team);
    t.vcap = S.vcap[s]; t.team_doubles = S.team_doubles[s]; t.flat = S.flat[s] ? 1 : 0; t.shared_doubles = S.shared[s];
}

// eri_teamc_kernel: the team's scratch holds E12, E34, R, G of one primitive quartet, then the accumulation block
static inline TeamSizes carve_teamc(TClass &t)
{
    const int LAB = t.La + t.Lb, L = LAB + t.Lc + t.Ld, NM = L / 2 + 1, XS = NM | 1;
    carve_team_shared(t, false);
    t.vcap = team_even(2 * t.nEab + 2 * t.nEcd + (L + 1) * (L + 2) + t.nTcd * (LAB + 1) * NM);      // E12, E34, R, G of one primitive quartet
    t.team_doubles = 2 * t.nT * XS + t.vcap + team_even(t.nacc) + team_even((t.nkap + 1) / 2);
    TeamSizes S{};
    for (int s = 0; s < 3; ++s) {
        S.vcap[s] = t.vcap; S.team_doubles[s] = t.team_doubles; S.shared[s] = t.shared_doubles; S.flat[s] = false;
        S.bytes[s] = ((size_t)t.shared_doubles + (size_t)(256 / TEAM_SIZES[s]) * t.team_doubles) * sizeof(double);
    }
    return S;
}

// lanes per quartet: 16 for the smallest classes; a wave while four quartets' tables fit about half of the LDS (two workgroups per
// CU); the whole workgroup beyond.  (Measured at N = 400, ERI kernels: 36 / 52 / 76 / 100 KB limit: 35.3 / 32.8 / 31.9 / 33 ms.)
// avail / bytes: by team_slot; soft64: the 64-lane limit in bytes; force: a size to take if it is instantiated and fits (0: none).
// Returns 0 when no team kernel takes the class.
static inline int choose_team(const bool avail[3], const size_t bytes[3], int nT, int nnzc, size_t soft64, int t16_nnz, int force)
{
    int team = 0;
    if (nT <= 16 && nnzc <= t16_nnz && avail[0]) team = 16;
    else if (avail[1] && bytes[1] <= soft64) team = 64;
    else if (avail[2] && bytes[2] <= ERI_LDS_MAX_BYTES) team = 256;
    else if (avail[1] && bytes[1] <= ERI_LDS_MAX_BYTES) team = 64;
    if (force == 16 || force == 64 || force == 256)
        if (avail[team_slot(force)] && bytes[team_slot(force)] <= ERI_LDS_MAX_BYTES) team = force;
    return team;
}

// a workgroup walks over several ket groups (shared staging once): enough workgroups to fill the chip, at most kpw_max groups each
// (measured at N = 400, ERI kernels: >= 65536 / 16384 / 4096 / 2048 / 1024 / 512 workgroups per launch aimed at:
// 36.0 / 32.8 / 28.3 / 26.8 / 26.5-27.1 / 27.9 ms).  Returns the workgroups along the ket axis.
static inline unsigned team_grid_x(int n_ket, int team, unsigned n_bra, long long kpw_div, long long kpw_max)
{
    const int NT = 256 / team;
    const long long groups = (n_ket + NT - 1) / NT;
    const long long kpw = std::max<long long>(1, std::min<long long>(kpw_max, groups * n_bra / kpw_div));
    return (unsigned)((groups + kpw - 1) / kpw);
}

}  // namespace tfe
