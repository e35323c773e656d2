// TEST INFRASTRUCTURE: the HIP-free parts of the context core behind a C interface for tests/test_ctx_plan.py: the owners of
// tf_ctx_plan.h (through owner_checks.h), the shard plans of tf_shard_plan.h, and tf::build_basis + tf::build_device_tables of
// tf_host.cpp (which build.sh compiles into this library).  No GPU code.
#include <cstdint>
#include <string>

#include "owner_checks.h"
#include "../../tuna_amd/csrc/tf_shard_plan.h"
#include "../../tuna_amd/csrc/tf_internal.h"
#include "../../tuna_amd/csrc/tf_eri_types.h"

namespace {
struct Tables { tf::Basis bs; tfk::DeviceTables t; std::string msg; };
template <class T, class U> void copy_as(const std::vector<U> &v, void *dst) { T *d = (T *)dst; for (size_t k = 0; k < v.size(); ++k) d[k] = (T)v[k]; }
}

extern "C" {

// ---- owners
int ctxm_refused(void) { return ctxm::REFUSED; }
void ctxm_counts(long long out[3]) { out[0] = tfctx::CB_COUNT; out[1] = ctxm::Streams::N_STREAMS; out[2] = ctxm::Streams::N_EVENTS; }
int ctxm_block_growth(int slot) { return ctxm::block_growth_check(slot); }
int ctxm_block_refusal(int k, int grow, int use_replace) { return ctxm::block_refusal_check(k, grow, use_replace); }
void ctxm_streams(int k, long long *out13) { ctxm::streams_run(k, out13); }
int ctxm_streams_verdict(int k, const long long *o13) { return ctxm::streams_verdict(k, o13); }
int ctxm_streams_names(void) { return ctxm::streams_names_check(); }
int ctxm_event_pairs(int pairs, int k) { return ctxm::event_pairs_check(pairs, k); }

// ---- shard plans: forced = 0 (TF_SHARD_PLAN not set), 1 "segments", 2 "shells"
void ctxm_shard_plan_pairs(int n_shells, const int32_t *dim, int layout, int world, int forced, int32_t *owner)
{
    static const char *const names[3] = {nullptr, "segments", "shells"};
    std::vector<int> d(dim, dim + n_shells), o;
    shard_plan_pairs(d, layout >= 1, world, names[forced], o);
    std::copy(o.begin(), o.end(), owner);
}
void ctxm_shard_plan(int n, const int64_t *weight, int world, int32_t *owner)
{
    std::vector<long long> w(weight, weight + n);
    std::vector<int> o;
    shard_plan(w, world, o);
    std::copy(o.begin(), o.end(), owner);
}

// ---- device tables of a basis.  The handle is null when the basis is refused.
void *ctxm_tables(int n, const double *origin, const int32_t *lmn, const int32_t *prim_off, const double *exps, const double *coefs, int exact_class)
{
    Tables *h = new Tables();
    h->msg = tf::build_basis(h->bs, n, origin, lmn, prim_off, exps, coefs);
    if (!h->msg.empty()) { delete h; return nullptr; }
    tf::build_device_tables(h->bs, exact_class != 0, h->t);
    return h;
}
void ctxm_tables_free(void *h) { delete (Tables *)h; }
// out = {shells, pairs, component pairs (ct_ix), classes, components, len sph_base, len sph_ptr, len sph_idx, len ct_pos, len ct_ord, len ct_sc}
void ctxm_tables_sizes(const void *h, long long out[11])
{
    const Tables &T = *(const Tables *)h;
    out[0] = (long long)T.t.hs.size(); out[1] = (long long)T.t.hp.size(); out[2] = (long long)T.t.ct_ix.size(); out[3] = (long long)T.t.class_pairs.size();
    out[4] = (long long)T.bs.c_lx.size(); out[5] = (long long)T.t.sph_base.size(); out[6] = (long long)T.t.sph_ptr.size(); out[7] = (long long)T.t.sph_idx.size();
    out[8] = (long long)T.t.ct_pos.size(); out[9] = (long long)T.t.ct_ord.size(); out[10] = (long long)T.t.ct_sc.size();
}
// which: 0 shells [n][5] (L, ncomp, comp_off, cart_off, full); 1 pairs [n][18] (A, B, La, Lb, npp, cls, nca, ncb, compoff_a, compoff_b,
// cartoff_a, cartoff_b, tab_off, pcls[5]); 2 pair_class; 3 class_pairs as [class, pair] rows in stored order; 4 ct_ix; 5 ct_pos; 6 ct_ord;
// 7 sph_base; 8 sph_ptr; 9 sph_idx; 10 components [n][3] (lx, ly, lz)  -- all int32;  20 ct_sc; 21 sph_val; 22 c_scale  -- double
void ctxm_tables_copy(const void *h, int which, void *dst)
{
    const Tables &T = *(const Tables *)h;
    int32_t *d = (int32_t *)dst;
    switch (which) {
    case 0:
        for (size_t i = 0; i < T.t.hs.size(); ++i) {
            const tfk::DShell &s = T.t.hs[i];
            const int32_t row[5] = {s.L, s.ncomp, s.comp_off, s.cart_off, T.bs.shells[i].full ? 1 : 0};
            std::copy(row, row + 5, d + 5 * i);
        }
        break;
    case 1:
        for (size_t i = 0; i < T.t.hp.size(); ++i) {
            const tfk::DPair &p = T.t.hp[i];
            const int32_t row[18] = {p.A, p.B, p.La, p.Lb, p.npp, p.cls, p.nca, p.ncb, p.compoff_a, p.compoff_b, p.cartoff_a, p.cartoff_b, p.tab_off,
                                     p.pcls[0], p.pcls[1], p.pcls[2], p.pcls[3], p.pcls[4]};
            std::copy(row, row + 18, d + 18 * i);
        }
        break;
    case 2: copy_as<int32_t>(T.t.pair_class, dst); break;
    case 3:
        for (size_t c = 0; c < T.t.class_pairs.size(); ++c)
            for (int p : T.t.class_pairs[c]) { *d++ = (int32_t)c; *d++ = p; }
        break;
    case 4: copy_as<int32_t>(T.t.ct_ix, dst); break;
    case 5: copy_as<int32_t>(T.t.ct_pos, dst); break;
    case 6: copy_as<int32_t>(T.t.ct_ord, dst); break;
    case 7: copy_as<int32_t>(T.t.sph_base, dst); break;
    case 8: copy_as<int32_t>(T.t.sph_ptr, dst); break;
    case 9: copy_as<int32_t>(T.t.sph_idx, dst); break;
    case 10:
        for (size_t i = 0; i < T.bs.c_lx.size(); ++i) { d[3 * i] = T.bs.c_lx[i]; d[3 * i + 1] = T.bs.c_ly[i]; d[3 * i + 2] = T.bs.c_lz[i]; }
        break;
    case 20: copy_as<double>(T.t.ct_sc, dst); break;
    case 21: copy_as<double>(T.t.sph_val, dst); break;
    case 22: copy_as<double>(T.bs.c_scale, dst); break;
    }
}

}
