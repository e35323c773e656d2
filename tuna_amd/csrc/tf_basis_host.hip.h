// tf_basis_host.hip.h -- the life of a context and of its basis: tf_create / tf_destroy / tf_last_error,
// tf_normalize, tf_set_basis (checks, tf::build_basis, tf::build_device_tables, the upload chain, one commit), the three getters, the
// tables of the parity-blocked layout, and the entry points that need a basis but no tensor: tf_one_electron, tf_cross_overlap,
// tf_eri_element.  Included by tf_device.hip below tf_ranks_host.hip.h; one translation unit.

// Tables of the parity-blocked layout for the output AOs of this build (tf_packed_host.h: build_layout) and their device copy.
// cls[k]: x/y parity class of output AO k (original order).
static int build_blocked_layout(tf_ctx *ctx, const std::vector<int> &cls)
{
    tfp::HostLayout &H = ctx->hl;
    // (several ranks: the walks of the Fock kernel are cut into parts -- tf_packed_host.h)
    int parts = ctx->world >= 4 ? 4 : (ctx->world >= 2 ? 2 : 1);
    if (const char *e = getenv("TF_JK_PARTS")) parts = std::max(1, std::min(8, atoi(e)));
    const std::string msg = tfp::build_layout(cls, parts, H);
    if (!msg.empty()) TF_FAIL(ctx, TF_EINVAL, "%s", msg.c_str());
    const int N = H.N, NW = H.NW;
    // device copy
    BLayout L{};
    L.N = N; L.NW = NW; L.RS = H.RS; L.NPtot = H.NPtot;
    std::vector<int> itab(BL_ITAB, 0);
    std::vector<long long> ltab(BL_LTAB, 0);
    for (int c = 0; c < 4; ++c) {
        itab[BL_CSTART + c] = H.cstart[c]; itab[BL_CSIZE + c] = H.csize[c]; itab[BL_GBASE + c] = H.gbase[c];
        ltab[BL_CBASE + c] = H.cbase[c]; ltab[BL_NP + c] = H.NP[c];
        for (int a = 0; a < 4; ++a) itab[BL_FULLSEC + 4 * c + a] = H.fullsec[c][a];
    }
    for (int b = 0; b < 5; ++b) itab[BL_WFIRST + b] = H.wfirst[b];
    auto up_i = [&](const std::vector<int> &h, const int **d) { return upload(ctx, h, const_cast<int **>(d), ctx->build_mem); };
    int rc;
    if ((rc = upload(ctx, ltab, const_cast<long long **>(&L.ltab), ctx->build_mem))) return rc;
    if ((rc = up_i(itab, &L.itab)) || (rc = up_i(H.ao, &L.ao)) || (rc = up_i(H.origI, &L.origI)) || (rc = up_i(H.clsI, &L.clsI)) || (rc = up_i(H.cntA, &L.cntA)) ||
        (rc = up_i(H.kap0, &L.kap0)) || (rc = up_i(H.kapF, &L.kapF)) || (rc = up_i(H.rpoff, &L.rpoff)) || (rc = up_i(H.chunk_c0, &L.chunk_c0)) ||
        (rc = up_i(H.chunk_width, &L.chunk_width)) || (rc = up_i(H.chunk_cls, &L.chunk_cls)) || (rc = up_i(H.chunk_of, &L.chunk_of)) ||
        (rc = up_i(H.gk, &L.gk)))
        return rc;
    if ((rc = upload(ctx, H.kinfo, const_cast<KInfo **>(&L.kinfo), ctx->build_mem))) return rc;
    ctx->bl = L;
    return TF_OK;
}

extern "C" {

tf_ctx *tf_create(int device, int rank, int world)
{
    // (GPU_MAX_HW_QUEUES -- more hardware queues for the concurrent launches of the tensor build -- belongs to the HOST application: it has
    // to be in the environment before the first HIP call of the process, and setenv from a library is not safe beside a threaded host's
    // getenv.  INTEGRATION.md recommends 16; the Python package sets it on import unless TUNA_NO_HWQ is set.)
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_create_error = std::string("no HIP device available (") + hipGetErrorString(e) + "); libtunafock has no CPU fallback";
        return nullptr;
    }
    if (device < 0 || device >= n || world < 1 || rank < 0 || rank >= world) {
        g_create_error = "tf_create: bad device ordinal or rank/world";
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) {
        g_create_error = "hipSetDevice failed";
        return nullptr;
    }
    tf_ctx *ctx = new tf_ctx();
    ctx->device = device; ctx->rank = rank; ctx->world = world;
    ++g_live_contexts;
    return ctx;
}

void tf_destroy(tf_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    free_eri(ctx);
    free_basis(ctx);
    tfscf::release(ctx->scf);
    for (auto &wsp : ctx->scf_batch) if (wsp) tfscf::release(*wsp);
    ctx->scf_batch.clear();
    tfdft::release(ctx->grid);
    ctx->prof.destroy();
    ctx->bstr.destroy();
    comm_release(ctx);
    ctx->blk.release();
    ctx->arena1e.release();
    delete ctx;
    if (--g_live_contexts == 0) tfcache::trim();      // the last context of the process: the cached blocks go back to the runtime
}

const char *tf_last_error(const tf_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int tf_normalize(int l, int m, int n, int nprim, const double *exps, double *coefs_inout, double *norm_out)
{
    if (l < 0 || m < 0 || n < 0 || nprim <= 0 || !exps || !coefs_inout || !norm_out) return TF_EINVAL;
    tf::normalize_ao(l, m, n, nprim, exps, coefs_inout, norm_out);
    return TF_OK;
}

int tf_set_basis(tf_ctx *ctx, int n_ao_cart, const double *origin, const int32_t *lmn, const int32_t *prim_off,
                 const double *exps, const double *coefs_raw)
{
    if (!ctx) return TF_EINVAL;
    if (!origin || !lmn || !prim_off || !exps || !coefs_raw) TF_FAIL(ctx, TF_EINVAL, "tf_set_basis: null argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    free_eri(ctx);
    free_basis(ctx);
    tfdft::release(ctx->grid);
    // Built and uploaded beside the context, committed below after the last upload: a refusal or a failed upload leaves the context as
    // free_basis left it (no basis), and `mem` gives its blocks back.
    tf::Basis bs;
    std::string msg = tf::build_basis(bs, n_ao_cart, origin, lmn, prim_off, exps, coefs_raw);
    if (!msg.empty()) TF_FAIL(ctx, msg.find("aligned") != std::string::npos ? TF_EGEOM : TF_EINVAL, "%s", msg.c_str());
    DeviceTables t;
    tf::build_device_tables(bs, getenv("TF_ERI_EXACT_CLASS") != nullptr, t);
    std::vector<double> boys;
    tf::boys_table(boys);
    DeviceBlocks mem;
    DShell *d_sh; DPair *d_pr; int8_t *d_lx, *d_ly, *d_lz; double *d_sc, *d_p, *d_Pz, *d_K, *d_E, *d_boys;
    int *d_cti, *d_ctp, *d_cto; double *d_cts;
    int *d_sb, *d_sp, *d_si; double *d_sv;
    int rc;
    if ((rc = upload(ctx, t.ct_ix, &d_cti, mem)) || (rc = upload(ctx, t.ct_pos, &d_ctp, mem)) || (rc = upload(ctx, t.ct_ord, &d_cto, mem)) ||
        (rc = upload(ctx, t.ct_sc, &d_cts, mem)) || (rc = upload(ctx, t.hs, &d_sh, mem)) || (rc = upload(ctx, t.hp, &d_pr, mem)) ||
        (rc = upload(ctx, bs.c_lx, &d_lx, mem)) || (rc = upload(ctx, bs.c_ly, &d_ly, mem)) || (rc = upload(ctx, bs.c_lz, &d_lz, mem)) ||
        (rc = upload(ctx, bs.c_scale, &d_sc, mem)) || (rc = upload(ctx, bs.pp_p, &d_p, mem)) || (rc = upload(ctx, bs.pp_Pz, &d_Pz, mem)) ||
        (rc = upload(ctx, bs.pp_K, &d_K, mem)) || (rc = upload(ctx, bs.epool, &d_E, mem)) || (rc = upload(ctx, boys, &d_boys, mem)) ||
        (rc = upload(ctx, t.sph_base, &d_sb, mem)) || (rc = upload(ctx, t.sph_ptr, &d_sp, mem)) || (rc = upload(ctx, t.sph_idx, &d_si, mem)) ||
        (rc = upload(ctx, t.sph_val, &d_sv, mem)))
        return rc;
    // commit
    ctx->basis_mem.held.swap(mem.held);
    ctx->bs = std::move(bs);
    ctx->db = DBasis{d_sh, d_pr, d_lx, d_ly, d_lz, d_sc, d_p, d_Pz, d_K, d_E, d_boys, d_sb, d_sp, d_si, d_sv, d_cti, d_ctp, d_cto, d_cts, nullptr, nullptr};
    ctx->host_pairs = std::move(t.hp);
    ctx->h_ct_ix = std::move(t.ct_ix); ctx->h_ct_ord = std::move(t.ct_ord); ctx->h_ct_sc = std::move(t.ct_sc);
    ctx->pair_class = std::move(t.pair_class); ctx->class_pairs = std::move(t.class_pairs);
    ctx->d_pairs = d_pr;
    ctx->have_basis = true;
    return TF_OK;
}

int tf_get_norms(const tf_ctx *ctx, double *norm, double *coefs_normalised)
{
    if (!ctx || !ctx->have_basis) return TF_EINVAL;
    if (norm) std::copy(ctx->bs.ao_norm.begin(), ctx->bs.ao_norm.end(), norm);
    if (coefs_normalised) std::copy(ctx->bs.ao_coef.begin(), ctx->bs.ao_coef.end(), coefs_normalised);
    return TF_OK;
}

int tf_dims(const tf_ctx *ctx, int *n_cart, int *n_sph, int *n_shell)
{
    if (!ctx || !ctx->have_basis) return TF_EINVAL;
    if (n_cart) *n_cart = ctx->bs.n_cart;
    if (n_sph) *n_sph = ctx->bs.n_sph;
    if (n_shell) *n_shell = (int)ctx->bs.shells.size();
    return TF_OK;
}

int tf_get_sph_matrix(const tf_ctx *ctx, double *U)
{
    if (!ctx || !ctx->have_basis || !U) return TF_EINVAL;
    std::vector<double> u;
    tf::dense_sph_matrix(ctx->bs, u);
    std::copy(u.begin(), u.end(), U);
    return TF_OK;
}

// ---- one-electron integrals -------------------------------------------------------------------------

int tf_one_electron(tf_ctx *ctx, int n_atoms, const double *atom_xyz, const double *atom_charge, const double *dipole_origin,
                    int spherical, double *S, double *T, double *V, double *D, double *Q)
{
    if (!ctx) return TF_EINVAL;
    if (!ctx->have_basis) TF_FAIL(ctx, TF_EINVAL, "tf_one_electron: call tf_set_basis first");
    if (n_atoms < 1 || n_atoms > 2 || !atom_xyz || !atom_charge || !dipole_origin || !S || !T || !V)
        TF_FAIL(ctx, TF_EINVAL, "tf_one_electron: bad arguments");
    for (int a = 0; a < n_atoms; ++a)
        if (atom_xyz[3 * a] != 0.0 || atom_xyz[3 * a + 1] != 0.0)
            TF_FAIL(ctx, TF_EGEOM, "Molecule is incorrectly aligned! Unable to calculate molecular integrals.");
    if (spherical && !ctx->bs.all_full) TF_FAIL(ctx, TF_EINVAL, "spherical output needs complete shells");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::string msg = tfone::one_electron(ctx->bs, n_atoms, atom_xyz, atom_charge, dipole_origin, spherical, S, T, V, D, Q, ctx->db.boys, &ctx->arena1e);
    if (!msg.empty()) TF_FAIL(ctx, TF_ENODEVICE, "%s", msg.c_str());
    return TF_OK;
}

int tf_cross_overlap(tf_ctx *ctx, int n2, const double *origin2, const int32_t *lmn2, const int32_t *prim_off2,
                     const double *exps2, const double *coefs_raw2, double *S_cross)
{
    if (!ctx) return TF_EINVAL;
    if (!ctx->have_basis) TF_FAIL(ctx, TF_EINVAL, "tf_cross_overlap: call tf_set_basis first");
    if (n2 < 1 || !origin2 || !lmn2 || !prim_off2 || !exps2 || !coefs_raw2 || !S_cross)
        TF_FAIL(ctx, TF_EINVAL, "tf_cross_overlap: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    tf::Basis other;
    std::string msg = tf::build_basis(other, n2, origin2, lmn2, prim_off2, exps2, coefs_raw2);
    if (!msg.empty()) TF_FAIL(ctx, TF_EINVAL, "%s", msg.c_str());
    msg = tfone::cross_overlap(ctx->bs, other, S_cross, &ctx->arena1e);
    if (!msg.empty()) TF_FAIL(ctx, TF_ENODEVICE, "%s", msg.c_str());
    return TF_OK;
}

int tf_eri_element(tf_ctx *ctx, const double *origin, const int32_t *lmn, const int32_t *prim_off, const double *exps,
                   const double *coefs_raw, double *value)
{
    if (!ctx) return TF_EINVAL;
    if (!origin || !lmn || !prim_off || !exps || !coefs_raw || !value) TF_FAIL(ctx, TF_EINVAL, "tf_eri_element: null argument");
    // A throw-away 4-AO context; (b0 b1|b2 b3) is element [0,1,2,3] of its Cartesian tensor.
    tf_ctx *tmp = tf_create(ctx->device, 0, 1);
    if (!tmp) TF_FAIL(ctx, TF_ENODEVICE, "%s", g_create_error.c_str());
    int rc = tf_set_basis(tmp, 4, origin, lmn, prim_off, exps, coefs_raw);
    if (!rc) rc = tf_build_eri(tmp, 0);
    const int32_t idx[4] = {0, 1, 2, 3};
    if (!rc) rc = tf_sample_eri(tmp, 1, idx, value);
    if (rc) ctx->err = tmp->err;
    tf_destroy(tmp);
    return rc;
}

}  // extern "C"
