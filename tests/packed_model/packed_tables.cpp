// TEST INFRASTRUCTURE: exposes the host table builders of the packed tensor layout (tuna_amd/csrc/tf_packed_host.h) to
// tests/test_packed_tables.py and tests/test_gpu_packed_tables.py, the buffer plan of the Fock build (tf_jk_plan.h) to
// tests/test_jk_plan.py and the LDS plans of the ERI kernels (tf_eri_plan.h) to tests/test_eri_plan.py.  Built by
// tests/packed_model/build.sh with g++ (no HIP, no GPU); nothing in the product links it.
#include <cstring>
#include "../../tuna_amd/csrc/tf_packed_host.h"
#include "../../tuna_amd/csrc/tf_jk_plan.h"
#include "../../tuna_amd/csrc/tf_eri_plan.h"

struct Handle {
    tfp::HostLayout H;
    tfp::RowTables rows;
    tfp::JKWork W;
    tfp::ConsumerTables CT;
    std::string err;
};

template <class T> static long long give(const std::vector<T> &v, void *out)
{
    if (out && !v.empty()) memcpy(out, v.data(), v.size() * sizeof(T));
    return (long long)v.size();
}
template <class T> static long long give(const T *p, size_t n, void *out)
{
    if (out) memcpy(out, p, n * sizeof(T));
    return (long long)n;
}

extern "C" {

// cls[N]: parity class of every AO (original order); shell_dim[n_shells]: AOs of every shell; my_pairs[n_my]: owned shell pairs
// (index A (A + 1) / 2 + B, A >= B); parts: parts of a cut walk; RB: rows of a group
void *ptm_build(int N, const int *cls, int parts, int n_shells, const int *shell_dim, int n_my, const int *my_pairs, int RB)
{
    Handle *h = new Handle();
    h->err = tfp::build_layout(std::vector<int>(cls, cls + N), parts, h->H);
    if (!h->err.empty()) return h;
    std::vector<tf::Pair> pairs;
    std::vector<int> off(n_shells, 0), dim(shell_dim, shell_dim + n_shells);
    for (int A = 0; A < n_shells; ++A) {
        if (A) off[A] = off[A - 1] + dim[A - 1];
        for (int B = 0; B <= A; ++B) { tf::Pair p{}; p.A = A; p.B = B; pairs.push_back(p); }
    }
    tfp::list_rows(pairs, off, dim, std::vector<int>(my_pairs, my_pairs + n_my), N, h->rows);
    tfp::pack_rows(h->H, false, h->rows);
    tfp::build_jk_work(h->H, h->rows, RB, h->W);
    tfp::build_class_rows(h->H, h->rows, h->CT);
    tfp::build_reduction_lists(h->H, h->rows, h->CT);
    return h;
}
void ptm_free(void *p) { delete (Handle *)p; }
const char *ptm_error(void *p) { return ((Handle *)p)->err.c_str(); }

long long ptm_const(const char *name)
{
    const std::string n(name);
    if (n == "SEG_PAD") return TF_SEG_PAD;
    if (n == "JBB") return TF_JKP_JBB;
    if (n == "GPW") return TF_JKP_GPW;
    if (n == "W") return TF_JKP_W;
    if (n == "CW") return TF_JKP_CW;
    if (n == "SEG") return TF_JKP_SEG;
    if (n == "RB1") return JKShape<1>::RB;
    if (n == "RB2") return JKShape<2>::RB;
    if (n == "sizeof_JKGroup") return sizeof(JKGroup);
    if (n == "sizeof_JKSuper") return sizeof(JKSuper);
    if (n == "sizeof_JKTask") return sizeof(JKTask);
    if (n == "ERI_LDS_MAX_BYTES") return (long long)tfe::ERI_LDS_MAX_BYTES;
    if (n == "ERI_THREADS") return TF_ERI_THREADS;
    if (n == "BLK_DOUBLES") return TF_BLK_DOUBLES;
    if (n == "CSR_DOUBLES") return TF_CSR_DOUBLES;
    if (n == "TEAM_LMAX") return TF_TEAM_LMAX;
    return -1;
}

// the buffer plan of the packed Fock build (tf_jk_plan.h).  in[12]: N, n_rows, NW, MP, RS, NPtot, n_groups[2], ypart_len[2], nseg[2];
// out[45]: Jrow, ypart, DI, DJ, Jt, cd[4], then per pass type (ND = 1, 2) the 18 members of JkPassPlan in the order of packed_tables.py
long long ptm_jk_plan(const long long *in, long long *out)
{
    JkPlanIn I;
    I.N = (int)in[0]; I.n_rows = in[1]; I.NW = (int)in[2]; I.MP = (int)in[3]; I.RS = (int)in[4]; I.NPtot = in[5];
    for (int t = 0; t < 2; ++t) { I.n_groups[t] = (int)in[6 + t]; I.ypart_len[t] = in[8 + t]; I.nseg[t] = (int)in[10 + t]; }
    const JkPlan P = jk_plan(I);
    long long *o = out;
    for (size_t v : {P.Jrow, P.ypart, P.DI, P.DJ, P.Jt, P.cd[0], P.cd[1], P.cd[2], P.cd[3]}) *o++ = (long long)v;
    for (const JkPassPlan &q : P.pass)
        for (size_t v : {q.DI0, q.DJ0, q.y0[0], q.y0[1], q.DIr, q.DJr, q.sP, q.sPp, q.sy, q.sJd, q.sDIc, q.sDIr, q.sDJc, q.sDJr, q.sJt, q.planeJd,
                         q.planeI, q.planeJ})
            *o++ = (long long)v;
    return o - out;
}

// ---- the LDS plans of the ERI kernels (tf_eri_plan.h), thin: integers in, the record's members out --------------------------------
// the class part of a QClass as EriBuild::launch_class fills it.  in[10]: La Lb Lc Ld nca ncb ncc ncd npp_ab npp_cd
static tfk::QClass eri_qclass(const int *in)
{
    tfk::QClass q{};
    q.La = in[0]; q.Lb = in[1]; q.Lc = in[2]; q.Ld = in[3];
    q.L = q.La + q.Lb + q.Lc + q.Ld; q.tsize = (q.L + 1) * (q.L + 2) / 2;
    q.nca = in[4]; q.ncb = in[5]; q.ncc = in[6]; q.ncd = in[7]; q.ncomp = q.nca * q.ncb * q.ncc * q.ncd;
    q.npp_ab = in[8]; q.npp_cd = in[9]; q.npq = q.npp_ab * q.npp_cd;
    q.nEab = (q.La + 1) * (q.Lb + 1) * (q.La + q.Lb + 1); q.nEcd = (q.Lc + 1) * (q.Ld + 1) * (q.Lc + q.Ld + 1);
    return q;
}
// family: 0 multi, 1 fact (tupG, tupXZ), 2 class, 3 component-per-lane.  out[20]: the members in the order of ERI_Q_FIELDS (packed_tables.py)
long long ptm_eri_carve(int family, const int *in, int tupG, int tupXZ, int *out)
{
    tfk::QClass q = eri_qclass(in);
    int stage = -1;
    if (family == 0) tfe::carve_multi(q);
    else if (family == 1) tfe::carve_fact(q, tupG, tupXZ);
    else if (family == 2) stage = tfe::carve_class(q) ? 1 : 0;
    else { q = tfk::QClass{}; tfe::carve_component_lane(q); }
    int *o = out;
    for (int v : {q.offR, q.offPref, q.offPQ, q.offRed, q.offEab, q.offEcd, q.offScale, q.offLmn, q.offBlk, q.offG, q.offTab, q.offCsr, q.lds_doubles,
                  q.PB, q.stride, q.G, q.ncp, q.tupG_off, q.tupXZ_off, stage})
        *o++ = v;
    return o - out;
}
int ptm_eri_lp_group(int lp) { return tfe::lp_group(lp); }
// pairs[n][5]: La Lb npp nE component pairs; out[6]: maxLp maxT maxLp1 maxE maxcomp maxnpp
static tfe::GroupStat eri_gs(const int *v) { tfe::GroupStat g; g.maxLp = v[0]; g.maxT = v[1]; g.maxLp1 = v[2]; g.maxE = v[3]; g.maxcomp = v[4]; g.maxnpp = v[5]; return g; }
void ptm_eri_group_stat(int n, const int *pairs, int *out)
{
    tfe::GroupStat g;
    for (int k = 0; k < n; ++k) tfe::group_stat(g, pairs[5 * k], pairs[5 * k + 1], pairs[5 * k + 2], pairs[5 * k + 3], pairs[5 * k + 4]);
    for (int v : {g.maxLp, g.maxT, g.maxLp1, g.maxE, g.maxcomp, g.maxnpp}) *out++ = v;
}
// in[21]: GroupStat of the bra group, of the ket group, bra contracted, ket contracted, nbt, xz, e, km members, packed, team_lmax,
// team_pqmax.  out[28]: the members of CFCaps in declaration order, then fit and gtab
long long ptm_eri_cfact(const int *in, int *out)
{
    const tfe::CFKnobs k{in[14], in[15], in[16]};
    const tfe::CFPlan P = tfe::carve_cfact(eri_gs(in), eri_gs(in + 6), in[12] != 0, in[13] != 0, k, in[17], in[18] != 0, in[19], in[20]);
    static_assert(sizeof(tfk::CFCaps) == 26 * sizeof(int), "CFCaps is 26 ints");
    memcpy(out, &P.caps, sizeof(tfk::CFCaps));
    out[26] = P.fit; out[27] = P.gtab;
    return 28;
}
// L4: La Lb Lc Ld; caps[ncaps][3]: capR capG capXZ of the launches the tuple can occur in; out[12]: LRec (tupG_off = 0); words: gsz + xz
long long ptm_eri_lrec(const int *L4, int ncaps, const int *caps, int *out, unsigned short *words)
{
    tfk::LRec r = tfe::lrec_sizes(L4[0], L4[1], L4[2], L4[3]);
    for (int k = 0; k < ncaps; ++k) {
        tfk::CFCaps c{};
        c.capR = caps[3 * k]; c.capG = caps[3 * k + 1]; c.capXZ = caps[3 * k + 2];
        tfe::lrec_limit(r, c);
    }
    r.tupG_off = 0; r.tupXZ_off = r.gsz;
    static_assert(sizeof(tfk::LRec) == 12 * sizeof(int), "LRec is 12 ints");
    memcpy(out, &r, sizeof(r));
    if (words) tfe::lrec_words(r, L4[0], L4[1], L4[2], L4[3], words);
    return r.gsz + r.xz;
}
// in[16]: La Lb Lc Ld nab ncd nkap nnzT nacc nout foff maxblk maxK nnzc nEab nEcd.  out[27]: oE12 oOffA oScA oOffK oTp oTk oTc oRowOff
// oCompW oOutW flat_off nflat, then by team size 16, 64, 256: vcap, team_doubles, shared_doubles, flat, bytes
long long ptm_eri_team(int per_class, const int *in, long long *out)
{
    tfk::TClass t{};
    t.La = in[0]; t.Lb = in[1]; t.Lc = in[2]; t.Ld = in[3];
    t.nTab = (t.La + 1) * (t.Lb + 1); t.nTcd = (t.Lc + 1) * (t.Ld + 1); t.nT = t.nTab * t.nTcd;
    t.nab = in[4]; t.ncd = in[5]; t.nkap = in[6]; t.nnzT = in[7]; t.nacc = in[8]; t.nout = in[9];
    t.nEab = in[14]; t.nEcd = in[15];
    const tfe::TeamSizes S = per_class ? tfe::carve_team(t, in[10], in[11], in[12], in[13]) : tfe::carve_teamc(t);
    long long *o = out;
    for (int v : {t.oE12, t.oOffA, t.oScA, t.oOffK, t.oTp, t.oTk, t.oTc, t.oRowOff, t.oCompW, t.oOutW, t.flat_off, t.nflat}) *o++ = v;
    for (int s = 0; s < 3; ++s) {
        tfk::TClass u = t;
        if (per_class) tfe::team_apply(u, S, tfe::TEAM_SIZES[s]);
        for (long long v : {(long long)u.vcap, (long long)u.team_doubles, (long long)u.shared_doubles, (long long)u.flat, (long long)S.bytes[s]}) *o++ = v;
    }
    return o - out;
}
int ptm_eri_choose_team(const int *avail, const long long *bytes, int nT, int nnzc, long long soft64, int t16_nnz, int force)
{
    const bool a[3] = {avail[0] != 0, avail[1] != 0, avail[2] != 0};
    const size_t b[3] = {(size_t)bytes[0], (size_t)bytes[1], (size_t)bytes[2]};
    return tfe::choose_team(a, b, nT, nnzc, (size_t)soft64, t16_nnz, force);
}
long long ptm_eri_team_grid_x(int n_ket, int team, long long n_bra, long long kpw_div, long long kpw_max)
{
    return tfe::team_grid_x(n_ket, team, (unsigned)n_bra, kpw_div, kpw_max);
}

// copies table `name` to out (if not null) and returns its number of elements; -1: no such table
long long ptm_get(void *p, const char *name, void *out)
{
    Handle *h = (Handle *)p;
    const tfp::HostLayout &H = h->H;
    const std::string n(name);
#define VEC(obj, f) if (n == #f) return give(obj.f, out)
#define ARR(obj, f, len) if (n == #f) return give(&obj.f[0], len, out)
#define SCALAR(obj, f) if (n == #f) { const long long v = (long long)obj.f; return give(&v, 1, out); }
    SCALAR(H, N) SCALAR(H, NW) SCALAR(H, RS) SCALAR(H, MC) SCALAR(H, KS) SCALAR(H, MP) SCALAR(H, NPtot) SCALAR(H, RLS)
    ARR(H, cstart, 4); ARR(H, csize, 4); ARR(H, corder, 4); ARR(H, wfirst, 5); ARR(H, gbase, 4); ARR(H, cbase, 4); ARR(H, NP, 4);
    if (n == "fullsec") return give(&H.fullsec[0][0], 16, out);
    VEC(H, cls); VEC(H, loc); VEC(H, sigma); VEC(H, ao); VEC(H, origI); VEC(H, clsI); VEC(H, cntA); VEC(H, kap0); VEC(H, kapF); VEC(H, rpoff);
    VEC(H, chunk_c0); VEC(H, chunk_width); VEC(H, chunk_cls); VEC(H, chunk_of); VEC(H, gk); VEC(H, kinfo); VEC(H, offE);
    VEC(h->rows, row_ij); VEC(h->rows, rowmap); VEC(h->rows, pair_first_row); VEC(h->rows, rowoff); VEC(h->rows, rowsec); VEC(h->rows, rowlen);
    SCALAR(h->rows, n_elems)
    VEC(h->W, groups); VEC(h->W, gfirst); VEC(h->W, supers); VEC(h->W, tasks); VEC(h->W, tasks_cd);
    ARR(h->W, bucket, 4); ARR(h->W, bucket_cd, 4); SCALAR(h->W, nseg) SCALAR(h->W, ypart_len)
    if (n == "jp") return give(&h->W.jp.sfirst[0], 10, out);
    VEC(h->CT, class_rows); VEC(h->CT, row_pos); ARR(h->CT, class_row_off, 5); VEC(h->CT, jptr); VEC(h->CT, jrows); VEC(h->CT, xorder);
#undef VEC
#undef ARR
#undef SCALAR
    return -1;
}
}
