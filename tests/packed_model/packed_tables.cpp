// TEST INFRASTRUCTURE: exposes the host table builders of the packed tensor layout (tuna_amd/csrc/tf_packed_host.h) to
// tests/test_packed_tables.py and tests/test_gpu_packed_tables.py.  Built by tests/packed_model/build.sh with g++ (no HIP, no GPU);
// nothing in the product links it.
#include <cstring>
#include "../../tuna_amd/csrc/tf_packed_host.h"
#include "../../tuna_amd/csrc/tf_jk_plan.h"

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
