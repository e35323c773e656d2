// tf_jk_host.hip.h -- the host side of the Fock build: the state of a tensor build, the passes over the packed and the tiles layout,
// the rows branch, the exchange step over the ranks, the public entry points, the profiling span.  Included by tf_device.hip (one
// translation unit: struct tf_ctx with its Fock state `jk` and the owner `build_mem`, DeviceBlocks, tf_malloc, upload, TF_FAIL and HIPCHK
// are defined there, above the include); kernels: tf_kernels.hip.h, tf_jkpacked.hip.h, tf_jktile.hip.h; buffer plan: tf_jk_plan.h.
// the pieces, who uses them, and the invariants (launches, events, memsets and copies of every call unchanged).
#pragma once

// ---- environment knobs of the Fock build: what they do, default, WHEN they are read ------------------------------------------------
// TF_JK_SERIAL          set: a pass launches on the caller's stream only, no fork / join events.  Unset.  packed: once per process (first
//                       pass with tasks); tiles: at EVERY pass
// TF_JK_ONE_LAUNCH      packed: fewer tasks than this go out as ONE launch of full-size workgroups (0: never).  12000.  Once (first pass with tasks)
// TF_JK_NOFUSE          set: two symmetric densities take two one-density passes, not the fused one.  Unset.  Once (first packed build)
// TF_JK_CLASS_DIAGONAL  "0": never use the class-diagonal task list.  On.  Once (first packed build)
// TF_JK_CD_NMIN         smallest N whose cycles test their densities for class-diagonality.  160.  Once (first packed build)
// TF_JKR_DBG            timing experiments of jk_reduce_kernel (1: exchange blocks only, 2: Jt blocks only).  0.  Once (first packed pass)
// TF_TILE_PF            tiles: 1 = the kernel variant with one step of tensor loads in flight.  2.  Once (first tiles pass with tasks)
// TF_TILE_WIDE_MIN      tiles: fewest symmetric densities that go through the wide (4 / 8) pass.  2.  Once (first tiles build)
// TF_TILE_PART_STEPS    tiles: steps per part of the wide pass's task list.  TT_STEPS_MAX.  Once (first wide list; tf_build_eri reads it
//                       for the stored list on its own, once)
// TF_JK_FORCE_NLC, TF_JK_FORCE_JB   rows: test hooks -- at least so many column chunks per thread; rows per workgroup (1, 2; 4 with one
//                       density).  Unset.  At EVERY rows build
// A "once" knob sits behind the function-local static of its accessor, which is called where the knob is used: the first use reads it.
// Tests set the knobs in child processes and, the per-call ones, in running processes.
struct JkKnobs {
    static int env_int(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }
    static bool serial_packed() { static const bool v = getenv("TF_JK_SERIAL") != nullptr; return v; }
    static bool serial_tiles() { return getenv("TF_JK_SERIAL") != nullptr; }
    // (measured: N = 60 99 -> 69 us per build, 118: 155 -> 108, 160: 202 -> 183, 200: equal, 300: 874 against 907)
    static int one_launch_below() { static const int v = env_int("TF_JK_ONE_LAUNCH", 12000); return v; }
    static bool no_fuse() { static const bool v = getenv("TF_JK_NOFUSE") != nullptr; return v; }
    static bool cd_off() { static const bool v = getenv("TF_JK_CLASS_DIAGONAL") && getenv("TF_JK_CLASS_DIAGONAL")[0] == '0'; return v; }
    // (the test is a kernel and a read-back, ~30 us: a build of a small tensor takes less than that in all -- N2/cc-pVTZ 70 us)
    static int cd_nmin() { static const int v = env_int("TF_JK_CD_NMIN", 160); return v; }
    static int jkr_dbg() { static const int v = env_int("TF_JKR_DBG", 0); return v; }
    static int tile_pf() { static const int v = env_int("TF_TILE_PF", 2); return v; }
    static int tile_wide_min() { static const int v = env_int("TF_TILE_WIDE_MIN", 2); return v; }
    static int tile_part_steps() { static const int v = std::min(TT_STEPS_MAX, std::max(1, env_int("TF_TILE_PART_STEPS", TT_STEPS_MAX))); return v; }
    static int force_nlc() { return env_int("TF_JK_FORCE_NLC", 0); }
    static int force_jb() { return env_int("TF_JK_FORCE_JB", 0); }
};

// The profiling span around the tensor kernels of one pass (tf_jk_profile): an event pair of ctx->prof, created on demand (if that
// fails the span is skipped silently); "before" is recorded on st by the constructor, "after" on st by end().
struct JkProfSpan {
    hipEvent_t after = nullptr;
    hipStream_t st;
    JkProfSpan(tf_ctx *ctx, hipStream_t s) : st(s)
    {
        hipEvent_t before, b;
        if (!ctx->prof_jk || !ctx->prof.next(before, b)) return;
        (void)hipEventRecord(before, st);
        after = b;
    }
    void end() { if (after) (void)hipEventRecord(after, st); }
};

// The eight pointer slots launch_jk takes: density q of the nd at P / J / K, the slots beyond nd repeat the last one
struct JkSlots {
    const double *p[8];
    double *j[8], *k[8];
    JkSlots(int nd, size_t nn, const double *P, double *J, double *K)
    {
        for (int q = 0; q < 8; ++q) { const size_t dq = (size_t)std::min(q, nd - 1); p[q] = P + dq * nn; j[q] = J + dq * nn; k[q] = K + dq * nn; }
    }
};

// ---- the Fock state of a tensor build: every block comes from ctx->build_mem and goes with it (free_eri) -------------------------------
// Buffers whose unwritten entries the reductions rely on are zeroed here, once.
static int jk_alloc_state(tf_ctx *ctx)
{
    const bool packed = ctx->layout >= 1, tiles = ctx->layout == 2;
    const tfp::HostLayout &H = ctx->hl;
    const size_t N = (size_t)ctx->N, ld = (size_t)ctx->ld, nn = N * N;
    auto alloc = [&](double **p, size_t doubles, bool zero) -> int {
        HIPCHK(ctx, ctx->build_mem.take((void **)p, doubles * sizeof(double)));
        if (zero) HIPCHK(ctx, hipMemset(*p, 0, doubles * sizeof(double)));
        return TF_OK;
    };
    int rc;
    tf_ctx::JkPacked &K = ctx->jk.packed;
    JkPlanIn in;
    in.N = ctx->N; in.n_rows = ctx->n_rows; in.NPtot = H.NPtot;
    if (packed) { in.NW = H.NW; in.MP = H.MP; in.RS = H.RS; }
    for (int t = 0; t < 2; ++t) { in.n_groups[t] = K.t[t].n_groups; in.ypart_len[t] = K.t[t].ypart_len; in.nseg[t] = K.t[t].nseg; }
    const JkPlan &P = K.plan = jk_plan(in);
    if ((rc = alloc(&ctx->jk.all.Jrow, P.Jrow, true))) return rc;
    if (tiles) {
        // partial sums of jk_tile_kernel (the lists' own buffers: tile_list_buffers) and the per-pass outputs of its reductions
        tf_ctx::JkTiles &T = ctx->jk.tiles;
        const size_t pml = (size_t)std::max(1, ctx->tiles.pm_len);
        if ((rc = alloc(&T.X, std::max<size_t>(1, 8 * nn), false)) || (rc = alloc(&T.Pm, 8 * pml, true)) ||
            (rc = alloc(&T.out, std::max<size_t>(1, 2 * 6 * 8 * nn), true)) || (rc = alloc(&T.JtTot, 8 * pml, true)))
            return rc;
    } else if (packed) {
        const size_t npr = (size_t)std::max<long long>(1, H.NPtot);    // padded pair index space
        if ((rc = alloc(&K.Psym, 2 * nn, false)) || (rc = alloc(&K.Pp, 2 * npr, true)) ||      // (Pp: the pad slots stay zero)
            (rc = alloc(&K.ypart, P.ypart, false)) || (rc = alloc(&K.DI, P.DI, false)) || (rc = alloc(&K.DJ, P.DJ, false)))
            return rc;
        // every region is zeroed once: the set of entries a pass writes does not depend on the density, and the reductions rely on the
        // entries no task writes being zero
        HIPCHK(ctx, hipMemset(K.DI, 0, P.DI * sizeof(double)));
        HIPCHK(ctx, hipMemset(K.DJ, 0, P.DJ * sizeof(double)));
        HIPCHK(ctx, hipMemset(K.ypart, 0, P.ypart * sizeof(double)));
        if ((rc = alloc(&K.Jt, P.Jt, false)) || (rc = alloc(&K.D, 2 * nn, false))) return rc;
    } else if ((rc = alloc(&ctx->jk.rows.Kp, 2 * std::max<size_t>(1, (size_t)ctx->n_rows) * 2 * ld, false)))
        return rc;
    const size_t npass = tiles ? 8 : 2;                             // densities of one call of tf_fock_jk that go through the tensor together
    tf_ctx::JkAll &A = ctx->jk.all;
    if ((rc = alloc(&A.Ppad, 2 * N * ld, false)) || (rc = alloc(&A.J, npass * nn, false)) || (rc = alloc(&A.K, npass * nn, false)) ||
        (rc = alloc(&A.P, npass * nn, false)))
        return rc;
    return TF_OK;
}

// ---- J/K ------------------------------------------------------------------------------------------

// nd = 1 or 2 densities in one pass over the tensor.  dP/dJ/dK: nd dense [N,N] device matrices each.
// One pass of jk_packed_kernel over ND densities (device, symmetric for the exchange part; X = what the D terms contract with) and the
// reductions; dDout[d]: the D matrix of density d.  Tables: set ND - 1.  Offsets and strides: the build's JkPlan.
extern "C++" {
template <int ND>
static int jk_packed_pass(tf_ctx *ctx, hipStream_t st, double *const *dDout, bool cd = false)
{
    const BLayout &L = ctx->bl;
    const int N = ctx->N;
    const tf_ctx::JkPacked &K = ctx->jk.packed;
    const tf_ctx::JKTables &T = K.t[ND - 1];
    const JkPassPlan &Q = K.plan.pass[ND - 1];
    JKStrides S{};
    const int MP = ctx->hl.MP;
    S.KS = ctx->hl.KS; S.MP = MP;
    S.planeJd = Q.planeJd; S.planeI = Q.planeI; S.planeJ = Q.planeJ;
    S.P = Q.sP; S.Pp = Q.sPp; S.y = Q.sy; S.Jd = Q.sJd;
    S.DIc = Q.sDIc; S.DIr = Q.sDIr; S.DJc = Q.sDJc; S.DJr = Q.sDJr;
    // cd: the class-diagonal task list with its own partial-sum buffers (launch_jk_packed decides)
    double *const pJrow = cd ? K.cd[JK_CD_JROW] : ctx->jk.all.Jrow;
    double *const pY = (cd ? K.cd[JK_CD_YPART] : K.ypart) + Q.y0[cd ? 1 : 0];
    const JKTask *const tasks = cd ? T.d_tasks_cd : T.d_tasks;
    const int n_tasks = cd ? T.n_tasks_cd : T.n_tasks;
    const int *const bucket = cd ? T.bucket_cd : T.bucket;
    double *DI0 = (cd ? K.cd[JK_CD_DI] : K.DI) + Q.DI0;
    double *DJ0 = (cd ? K.cd[JK_CD_DJ] : K.DJ) + Q.DJ0;
    double *DIc = DI0, *DIr = DI0 + Q.DIr, *DJc = DJ0, *DJr = DJ0 + Q.DJr;
    if (n_tasks > 0) {
        JkProfSpan span(ctx, st);
        // one launch per workgroup size; the launches are independent (disjoint tasks): the smaller ones go to side streams so that
        // their ramp-up and tail overlap the big one (fork / join on events; TF_JK_SERIAL=1: all on the caller's stream)
        int n_launch = 0;
        for (int b = 0; b < 3; ++b) n_launch += (bucket[b + 1] > bucket[b] && (TF_JKP_W >> b) >= 1) ? 1 : 0;
        // Few tasks (small tensors: N2/cc-pVTZ has 1 400): ONE launch of full-size workgroups over all of them -- the idle waves of the
        // narrower tasks cost nothing on a chip the build cannot fill, two launches and the fork / join events of the side streams do
        // (a Fock build at N = 60 is ~90 us of launches, not of work)
        // (one rank only: the rows of a rank of several are short runs of j -- mostly one group per super-group, three of four waves idle
        // in the barriers of a LONG walk; measured at N = 400 on 8 ranks: 0.72 ms per local build in one launch against 0.46 ms in three)
        // (a rank of several only when its super-groups are full -- the whole-shell plan: >= 24 rows per super-group on average; 0.382 -> 0.363 ms
        // per local build on 8 ranks.  Under the segment plan a rank's super-groups hold a few rows each: see above.)
        const bool full_supers = T.n_supers > 0 && ctx->n_rows >= 24LL * T.n_supers;
        const bool one_launch = JkKnobs::one_launch_below() > n_tasks && n_launch > 1 && (ctx->world == 1 || full_supers);
        const bool fork = !JkKnobs::serial_packed() && !one_launch && ctx->bstr.live && n_launch > 1;
        if (fork) (void)hipEventRecord(ctx->bstr.sev[0], st);
        int side = 0;
        bool first = true;
        if (one_launch)
            hipLaunchKernelGGL((jk_packed_kernel<ND>), dim3((unsigned)n_tasks), dim3(64 * TF_JKP_W), 0, st, ctx->d_eri(), T.d_groups,
                               T.d_supers, tasks, L, L.kinfo, K.Psym, K.Pp, pJrow, pY, DIc, DIr, DJc, DJr, S);
        for (int b = 0; b < 3 && !one_launch; ++b) {
            const int t0 = bucket[b], t1 = bucket[b + 1];
            if (!(t1 > t0 && (TF_JKP_W >> b) >= 1)) continue;
            hipStream_t ls = st;
            if (fork && !first) {
                ++side;
                ls = ctx->bstr.streams[side];
                (void)hipStreamWaitEvent(ls, ctx->bstr.sev[0], 0);
            }
            first = false;
            hipLaunchKernelGGL((jk_packed_kernel<ND>), dim3((unsigned)(t1 - t0)), dim3(64 * (TF_JKP_W >> b)), 0, ls, ctx->d_eri(), T.d_groups,
                               T.d_supers, tasks + t0, L, L.kinfo, K.Psym, K.Pp, pJrow, pY, DIc, DIr, DJc, DJr, S);
            if (ls != st) {
                (void)hipEventRecord(ctx->bstr.sev[side], ls);
                (void)hipStreamWaitEvent(st, ctx->bstr.sev[side], 0);
            }
        }
        span.end();
    }
    JKReduce R{};
    R.ypart = pY; R.sy = S.y; R.supers = T.d_supers; R.MC = ctx->hl.MC; R.MP = MP; R.planeI = S.planeI; R.planeJ = S.planeJ; R.nseg = T.nseg; R.jp = T.jp;
    R.Jt = K.Jt; R.sJt = Q.sJt;
    R.DIc = DIc; R.sDIc = S.DIc; R.DIr = DIr; R.sDIr = S.DIr; R.DJc = DJc; R.sDJc = S.DJc; R.DJr = DJr; R.sDJr = S.DJr;
    R.gfirst = T.d_gfirst; R.jptr = K.jptr; R.jrows = K.jrows; R.row_ij = ctx->d_row_ij; R.xorder = K.xorder;
    for (int d = 0; d < ND; ++d) R.D[d] = dDout[d];
    R.dbg = JkKnobs::jkr_dbg();
    const unsigned nblk = (unsigned)ND * ((unsigned)N * ((N + 127) / 128) + (unsigned)T.jp.bfirst[4] * T.nseg);
    hipLaunchKernelGGL(jk_reduce_kernel, dim3(nblk), dim3(TF_JKR_THREADS), 0, st, R, L);
    return TF_OK;
}
}  // extern "C++"

// nonsym[d] != 0: density d is not symmetric -- two passes (K = D(P^T) + D(P)^T); nullptr = all symmetric.
// try_cd: the caller expects class-diagonal densities (the native SCF cycles: theirs usually are).
static int launch_jk_packed(tf_ctx *ctx, int nd, const double *const *dP, double *const *dJ, double *const *dK, hipStream_t st,
                            const int *nonsym, bool try_cd)
{
    const BLayout &L = ctx->bl;
    const int N = ctx->N;
    const size_t nn = (size_t)N * N;
    tf_ctx::JkPacked &K = ctx->jk.packed;
    const JkPlan &P = K.plan;
    const dim3 gN((N * N + 255) / 256), b256(256);
    // Class-diagonal densities (what an SCF cycle of a diatomic without a transverse field produces: no element between AOs of
    // different x/y parity) need a quarter fewer tasks -- see JKTables::d_tasks_cd.  Only when the caller expects them (try_cd: the
    // test costs a small kernel and one 16-byte read-back per call) and only when no density of the call
    // has an element between two classes above 1e-14 of its largest element -- the threshold under which the blocked eigensolver
    // (tf_scf.hip.h) already treats such elements as zero.  With exact zeros there (densities built from class-pure orbitals) the skipped
    // products are exact zeros and J, K come out bit for bit the same; DIIS mixtures that carry 1e-16 of a host-made guess differ by that.
    bool cd = false;
    {
        const bool cd_on = !JkKnobs::cd_off(), cd_size = N >= JkKnobs::cd_nmin();
        bool any_general = false;
        for (int d = 0; d < nd; ++d) any_general = any_general || (nonsym && nonsym[d]);
        if (try_cd && cd_on && cd_size && !any_general && K.t[0].n_tasks_cd < K.t[0].n_tasks) {
            if (!K.cdflag) HIPCHK(ctx, ctx->build_mem.take((void **)&K.cdflag, 2 * sizeof(unsigned long long)));
            cd = true;
            for (int d = 0; d < nd && cd; ++d) {                   // (per density: the threshold is relative to ITS largest element)
                HIPCHK(ctx, hipMemsetAsync(K.cdflag, 0, 2 * sizeof(unsigned long long), st));
                hipLaunchKernelGGL(class_cross_max_kernel, dim3((unsigned)N), dim3(256), 0, st, dP[d], L, K.cdflag);
                double h[2] = {0.0, 1.0};
                HIPCHK(ctx, hipMemcpyAsync(h, K.cdflag, sizeof(h), hipMemcpyDeviceToHost, st));
                HIPCHK(ctx, hipStreamSynchronize(st));
                cd = std::isfinite(h[0]) && h[0] < 1e299 && h[1] <= 1e-14 * h[0];
            }
            if (cd && !K.cd[0]) {                                  // the second set of partial-sum buffers: zeroed once, like the first
                for (int q = 0; q < 4; ++q) {
                    if (!(K.cd[q] = ctx->build_mem.alloc(P.cd[q]))) {                         // no room: the full list then
                        for (int u = 0; u < q; ++u) { ctx->build_mem.release(K.cd[u]); K.cd[u] = nullptr; }
                        cd = false;
                        break;
                    }
                    HIPCHK(ctx, hipMemsetAsync(K.cd[q], 0, P.cd[q] * sizeof(double), st));
                }
            }
            if (cd) ++ctx->jk_cd_passes; else ++ctx->jk_cd_declined;
        }
    }
    double *const pJrow = cd ? K.cd[JK_CD_JROW] : ctx->jk.all.Jrow;
    if (!JkKnobs::no_fuse() && nd == 2 && !(nonsym && (nonsym[0] || nonsym[1]))) {
        // two symmetric densities (UHF alpha / beta): one pass over the tensor, groups of 4 rows x 2 densities
        const JkPassPlan &Q = P.pass[1];
        for (int d = 0; d < 2; ++d)
            hipLaunchKernelGGL(pack_density_kernel, gN, b256, 0, st, dP[d], L, 0, K.Psym + d * Q.sP, K.Pp + d * Q.sPp);
        double *dD[2] = {K.D, K.D + nn};
        int rc = jk_packed_pass<2>(ctx, st, dD, cd);
        if (rc) return rc;
        for (int d = 0; d < 2; ++d)
            hipLaunchKernelGGL(jk_packed_final_kernel, gN, b256, 0, st, dD[d], dD[d], pJrow + d * Q.sJd, Q.planeJd,
                               ctx->hl.KS, ctx->hl.MP, K.Jt + d * Q.sJt, K.t[1].nseg, ctx->d_rowmap, L, dJ[d], dK[d]);
        return TF_OK;
    }
    for (int d = 0; d < nd; ++d)                                 // one density per pass over the packed tensor
      for (int pass = 0; pass < ((nonsym && nonsym[d]) ? 2 : 1); ++pass) {
        const bool general = nonsym && nonsym[d];
        double *dD = (pass == 0) ? K.D : K.D + nn;
        hipLaunchKernelGGL(pack_density_kernel, gN, b256, 0, st, dP[d], L, (general && pass == 0) ? 1 : 0, K.Psym, K.Pp);
        double *dDp[1] = {dD};
        int rc = jk_packed_pass<1>(ctx, st, dDp, cd);
        if (rc) return rc;
        if (general && pass == 0) continue;
        hipLaunchKernelGGL(jk_packed_final_kernel, gN, b256, 0, st, K.D, dD, pJrow, P.pass[0].planeJd, ctx->hl.KS, ctx->hl.MP, K.Jt,
                           K.t[0].nseg, ctx->d_rowmap, L, dJ[d], dK[d]);
      }
    return TF_OK;
}

// Fock build from the tiles layout (tf_jktile.hip.h): pack -> jk_tile_kernel beside jk_edge_kernel -> jk_tile_reduce_kernel ->
// jk_tile_final_kernel.  One density per pass (a non-symmetric one: two passes, K = D(P^T) + D(P)^T), or -- symmetric densities only --
// up to eight per pass: densities = columns of the B operands of the matrix-core products (ND = 4 or 8; fewer: zero columns).
extern "C++" {
// the partial-sum buffers of a list for nd densities per pass
static int tile_list_buffers(tf_ctx *ctx, tf_ctx::TileList &D, int nd)
{
    if (D.nd_cap >= nd) return TF_OK;
    const std::pair<double **, size_t> bufs[5] = {{&D.DJ, (size_t)D.dj_len}, {&D.Jt, (size_t)D.jt_len}, {&D.Jd, (size_t)D.jd_len},
                                                  {&D.DIk, (size_t)D.n_di * 64}, {&D.DIl, (size_t)D.n_di * 16}};
    for (const auto &b : bufs) HIPCHK(ctx, ctx->build_mem.take((void **)b.first, std::max<size_t>(1, b.second * nd) * sizeof(double)));
    D.nd_cap = nd;
    return TF_OK;
}
// device copy of a task list
static int tile_list_upload(tf_ctx *ctx, const tft::TaskList &TL, bool own_shapes, tf_ctx::TileList &D)
{
    DeviceBlocks &mem = ctx->build_mem;
    int rc;
    if (own_shapes && ((rc = upload(ctx, TL.pairs, &D.d_pairs, mem)) || (rc = upload(ctx, TL.runs, &D.d_runs, mem)))) return rc;   // (the shapes of the DJ vectors differ with the strip height)
    if ((rc = upload(ctx, TL.tasks, &D.d_tasks, mem)) || (rc = upload(ctx, TL.itask_ptr, &D.d_itask_ptr, mem)) || (rc = upload(ctx, TL.itasks, &D.d_itasks, mem))) return rc;
    D.n_tasks = (int)TL.tasks.size(); D.ksub = TL.ksub; D.n_di = TL.n_di; D.dj_len = TL.dj_len; D.jd_len = TL.jd_len; D.jt_len = TL.jt_len;
    for (int b = 0; b <= TT_W; ++b) D.bucket[b] = TL.bucket[b];
    return TF_OK;
}

// one pass over the tensor for the ND densities in the tiles state's X / Pm (packed by the caller); `out`: [6][ND][N][N]
template <int ND>
static int jk_tiles_pass(tf_ctx *ctx, tf_ctx::TileList &D, hipStream_t st, double *out)
{
    const int N = ctx->N;
    const size_t nn = (size_t)N * N;
    const tft::Tables &TT = ctx->tiles;
    const tf_ctx::JkTiles &Z = ctx->jk.tiles;
    int rc = tile_list_buffers(ctx, D, ND);
    if (rc) return rc;
    int jt_rows = 0;
    for (int p = 0; p < TT.npair; ++p) jt_rows += ctx->hl.csize[TT.pa[p]];
    const size_t edge_lds = (size_t)(2 + 3 * TT_EDGE_WAVES) * N * sizeof(double), red_lds = std::max((size_t)2 * TT_RED_WAVES * N, (size_t)TT_RED_WAVES * 64 * std::max(TT_RED_CT, ND)) * sizeof(double);
    if (std::max(edge_lds, red_lds) > ctx->tile_lds_set) {                // (beyond the default 64 KB per workgroup: N > 580)
        if (std::max(edge_lds, red_lds) > (size_t)160 * 1024 - 1024) TF_FAIL(ctx, TF_EINVAL, "N = %d exceeds the LDS rows of the tiles layout's reductions", N);
        const int want = (int)std::max(edge_lds, red_lds);
        HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&jk_edge_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, want));
        HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&jk_edge_kernel<4>), hipFuncAttributeMaxDynamicSharedMemorySize, want));
        HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&jk_edge_kernel<8>), hipFuncAttributeMaxDynamicSharedMemorySize, want));
        HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&jk_tile_reduce_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, want));
        HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&jk_tile_reduce_kernel<4>), hipFuncAttributeMaxDynamicSharedMemorySize, want));
        HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&jk_tile_reduce_kernel<8>), hipFuncAttributeMaxDynamicSharedMemorySize, want));
        ctx->tile_lds_set = (size_t)want;
    }
    TJArgs A{};
    A.DJ = D.DJ; A.Jt = D.Jt; A.Jd = D.Jd; A.DIk = D.DIk; A.DIl = D.DIl; A.sJt = (size_t)D.jt_len; A.sDIk = (size_t)D.n_di * 64; A.sDIl = (size_t)D.n_di * 16;
    A.N = N; A.pm_len = TT.pm_len;
    TEArgs E{};
    E.edge_base = TT.edge_base; E.N = N; E.tab = Z.tvtab; E.EJ = out + 5 * ND * nn; E.ED = out + 2 * ND * nn; E.EDT = out + 3 * ND * nn; E.sE = nn;
    const bool fork = ctx->bstr.live && !JkKnobs::serial_tiles();
    if (D.n_tasks > 0) {
        JkProfSpan span(ctx, st);
        if (fork) (void)hipEventRecord(ctx->bstr.sev[0], st);
        // ONE launch of full-size workgroups over all tasks (measured at N = 400: 1.57 ms against 1.82 for one launch per workgroup size
        // on side streams -- loads only); the idle waves of the narrower tasks wait in the task's barriers
        const int pf_env = JkKnobs::tile_pf();
        const dim3 grid((unsigned)D.n_tasks), block(64 * TT_W);
#define TF_TJ_LAUNCH(NDV, MBV, PFV) hipLaunchKernelGGL((jk_tile_kernel<NDV, MBV, PFV>), grid, block, 0, st, ctx->d_eri(), D.d_tasks, Z.X, Z.Pm, A)
        if constexpr (ND == 1) {
            if (D.ksub == 16) { if (pf_env == 1) TF_TJ_LAUNCH(1, 1, 1); else TF_TJ_LAUNCH(1, 1, 2); }
            else if (D.ksub == 32) { if (pf_env == 1) TF_TJ_LAUNCH(1, 2, 1); else TF_TJ_LAUNCH(1, 2, 2); }
            else TF_TJ_LAUNCH(1, 4, 1);
        } else {
            if (D.ksub != 16) TF_FAIL(ctx, TF_EINVAL, "tiles layout: the wide pass needs the list of 16-row strips");
            if (pf_env == 1) TF_TJ_LAUNCH(ND, 1, 1); else TF_TJ_LAUNCH(ND, 1, 2);
        }
#undef TF_TJ_LAUNCH
        span.end();
    }
    {
        // the edge elements beside the tile launch
        hipStream_t ls = st;
        if (fork && D.n_tasks > 0) { ls = ctx->bstr.streams[1]; (void)hipStreamWaitEvent(ls, ctx->bstr.sev[0], 0); }
        hipLaunchKernelGGL((jk_edge_kernel<ND>), dim3((unsigned)N, (unsigned)ND), dim3(64 * TT_EDGE_WAVES), edge_lds, ls, ctx->d_eri(), Z.X, D.d_runs, E);
        if (ls != st) { (void)hipEventRecord(ctx->bstr.sev[1], ls); (void)hipStreamWaitEvent(st, ctx->bstr.sev[1], 0); }
    }
    TRArgs R{};
    R.itask_ptr = D.d_itask_ptr; R.itasks = D.d_itasks; R.jlist_ptr = Z.jlist_ptr; R.clsI = ctx->bl.clsI;
    R.DJ = D.DJ; R.Jt = D.Jt; R.Jd = D.Jd; R.DIk = D.DIk; R.DIl = D.DIl; R.T = ctx->d_eri(); R.X = Z.X;
    R.sJt = A.sJt; R.sDIk = A.sDIk; R.sDIl = A.sDIl; R.sO = nn;
    R.Dj = out; R.Di = out + (size_t)ND * nn; R.JD = out + (size_t)4 * ND * nn; R.JtTot = Z.JtTot;
    R.edge_base = TT.edge_base; R.N = N; R.ksub = D.ksub; R.npair = TT.npair; R.nd = ND; R.pm_len = TT.pm_len; R.tab = Z.tvtab;
    R.jt_rows = jt_rows;
    const unsigned nblk = ND == 1 ? (unsigned)(5 * N + jt_rows) : (unsigned)(4 * N) + (unsigned)ND * (unsigned)(N + jt_rows);
    hipLaunchKernelGGL(jk_tile_reduce_kernel<ND>, dim3(nblk), dim3(TT_RED_THREADS), red_lds, st, D.d_tasks, D.d_pairs, D.d_runs, Z.jlist, R);
    return TF_OK;
}
}  // extern "C++"

static int launch_jk_tiles(tf_ctx *ctx, int nd, const double *const *dP, double *const *dJ, double *const *dK, hipStream_t st, const int *nonsym)
{
    const int N = ctx->N;
    const size_t nn = (size_t)N * N, pml = (size_t)std::max(1, ctx->tiles.pm_len);
    tf_ctx::JkTiles &Z = ctx->jk.tiles;
    const dim3 gN((unsigned)((nn + 255) / 256)), b256(256);
    auto final_launch = [&](const double *o0, const double *o1, int ndp, int d, const double *jtt, double *J, double *K) {
        TFArgs F{};                                                          // out sets: [6][ndp][N][N]; D of the first pass, D2 of the last
        F.Dj = o0 + (size_t)(0 * ndp + d) * nn; F.Di = o0 + (size_t)(1 * ndp + d) * nn; F.ED = o0 + (size_t)(2 * ndp + d) * nn; F.EDT = o0 + (size_t)(3 * ndp + d) * nn;
        F.Dj2 = o1 + (size_t)(0 * ndp + d) * nn; F.Di2 = o1 + (size_t)(1 * ndp + d) * nn; F.ED2 = o1 + (size_t)(2 * ndp + d) * nn; F.EDT2 = o1 + (size_t)(3 * ndp + d) * nn;
        F.JD = o1 + (size_t)(4 * ndp + d) * nn; F.EJ = o1 + (size_t)(5 * ndp + d) * nn; F.JtTot = jtt; F.tab = Z.tvtab;
        hipLaunchKernelGGL(jk_tile_final_kernel, gN, b256, 0, st, F, ctx->bl, J, K);
    };
    bool any_general = false;
    for (int d = 0; d < nd; ++d) any_general = any_general || (nonsym && nonsym[d]);
    if (nd >= JkKnobs::tile_wide_min() && nd >= 2 && !any_general) {
        // the list of 16-row strips (one row block per wave: the registers hold ND accumulator sets), built at first use
        if (!Z.tlw.d_tasks) {
            const tft::TaskList *TL = &ctx->tsubw;
            if (ctx->ksub1 == 16) TL = &ctx->tsub1;
            else {
                const std::string e = tft::build_list(ctx->tclass, ctx->tiles, ctx->trows, 16, JkKnobs::tile_part_steps(), ctx->tsubw);
                if (!e.empty()) TF_FAIL(ctx, TF_EINVAL, "%s", e.c_str());
            }
            int rc = tile_list_upload(ctx, *TL, true, Z.tlw);
            if (rc) return rc;
        }
        for (int d0 = 0; d0 < nd;) {
            const int left = nd - d0, ndp = left > 4 ? 8 : 4, n = std::min(left, ndp);
            for (int d = 0; d < n; ++d)
                hipLaunchKernelGGL(pack_density_tiles_kernel, gN, b256, 0, st, dP[d0 + d], ctx->bl, ctx->tv, 0, Z.X + (size_t)d * nn, Z.Pm + (size_t)d * pml);
            if (n < ndp) {                                                   // empty columns
                HIPCHK(ctx, hipMemsetAsync(Z.X + (size_t)n * nn, 0, (size_t)(ndp - n) * nn * sizeof(double), st));
                HIPCHK(ctx, hipMemsetAsync(Z.Pm + (size_t)n * pml, 0, (size_t)(ndp - n) * pml * sizeof(double), st));
            }
            int rc = ndp == 8 ? jk_tiles_pass<8>(ctx, Z.tlw, st, Z.out) : jk_tiles_pass<4>(ctx, Z.tlw, st, Z.out);
            if (rc) return rc;
            for (int d = 0; d < n; ++d) final_launch(Z.out, Z.out, ndp, d, Z.JtTot + (size_t)d * pml, dJ[d0 + d], dK[d0 + d]);
            d0 += n;
        }
        return TF_OK;
    }
    for (int d = 0; d < nd; ++d) {
        const bool general = nonsym && nonsym[d];
        for (int pass = 0; pass < (general ? 2 : 1); ++pass) {
            double *out = Z.out + (size_t)pass * 6 * nn;
            hipLaunchKernelGGL(pack_density_tiles_kernel, gN, b256, 0, st, dP[d], ctx->bl, ctx->tv, (general && pass == 0) ? 1 : 0, Z.X, Z.Pm);
            int rc = jk_tiles_pass<1>(ctx, Z.tl1, st, out);
            if (rc) return rc;
            if (general && pass == 0) continue;
            final_launch(Z.out, out, 1, 0, Z.JtTot, dJ[d], dK[d]);
        }
    }
    return TF_OK;
}

// try_cd: see launch_jk_packed (the native cycles pass true, everyone else false)
static int launch_jk(tf_ctx *ctx, int nd, const double *const *dP, double *const *dJ, double *const *dK, hipStream_t st,
                     const int *nonsym = nullptr, bool try_cd = false)
{
    if (ctx->layout == 2) return launch_jk_tiles(ctx, nd, dP, dJ, dK, st, nonsym);
    if (ctx->layout == 1) return launch_jk_packed(ctx, nd, dP, dJ, dK, st, nonsym, try_cd);
    const int N = ctx->N, ld = ctx->ld;
    const tf_ctx::JkAll &A = ctx->jk.all;
    double *const Kp = ctx->jk.rows.Kp;
    const double *Ppad[2] = {dP[0], nd > 1 ? dP[1] : dP[0]};
    if (ld != N) {
        for (int d = 0; d < nd; ++d) {
            double *dst = A.Ppad + (size_t)d * N * ld;
            hipLaunchKernelGGL(pad_matrix_kernel, dim3((N * ld + 255) / 256), dim3(256), 0, st, dP[d], dst, N, ld);
            Ppad[d] = dst;
        }
    }
    if (ctx->n_rows > 0) {
        const int npair = ld / 2;
        // rows per workgroup: share each P tile among JB rows, but keep >= ~2 workgroups per CU in flight
        int JB = (ctx->n_rows >= 4 * 2048) ? 4 : (ctx->n_rows >= 2 * 2048 ? 2 : 1);
        if (nd == 2 && JB == 4) JB = 2;                         // register budget
        int nlc = (npair <= TF_JK_THREADS) ? 1 : (npair <= 2 * TF_JK_THREADS ? 2 : 4);
        // test hooks (tests/test_gpu_sharded.py): exercise the variants that only N > 512 would select
        nlc = std::max(nlc, JkKnobs::force_nlc());
        { const int f = JkKnobs::force_jb(); if (f == 1 || f == 2 || (f == 4 && nd == 1)) JB = f; }
        // instantiated combinations: (NLC 4, one density) up to JB 2; (NLC 4, two densities) JB 1 -- the grid below must match
        if (nlc == 4 && nd == 1 && JB == 4) JB = 2;
        if (nlc == 4 && nd == 2) JB = 1;
        const size_t smem = (size_t)(2 * nd * JB * N + 4 * TF_JK_THREADS) * sizeof(double);
        const dim3 grid((unsigned)((ctx->n_rows + JB - 1) / JB)), block(TF_JK_THREADS);
        JkProfSpan span(ctx, st);
#define TF_JK_LAUNCH(NLC, JBV, NDV)                                                                                         \
        hipLaunchKernelGGL((jk_rows_kernel<NLC, JBV, NDV>), grid, block, smem, st, ctx->d_eri(), ctx->d_row_ij, ctx->n_rows, N, ld, \
                           Ppad[0], Ppad[1], A.Jrow, Kp)
        if (npair > 4 * TF_JK_THREADS) TF_FAIL(ctx, TF_EINVAL, "N = %d exceeds the J/K kernel's row length limit (2048)", N);
        if (nd == 1) {
            if (nlc == 1) {
                if (JB == 4) TF_JK_LAUNCH(1, 4, 1); else if (JB == 2) TF_JK_LAUNCH(1, 2, 1); else TF_JK_LAUNCH(1, 1, 1);
            } else if (nlc == 2) {
                if (JB == 4) TF_JK_LAUNCH(2, 4, 1); else if (JB == 2) TF_JK_LAUNCH(2, 2, 1); else TF_JK_LAUNCH(2, 1, 1);
            } else {
                if (JB >= 2) TF_JK_LAUNCH(4, 2, 1); else TF_JK_LAUNCH(4, 1, 1);
            }
        } else {
            if (nlc == 1) {
                if (JB == 2) TF_JK_LAUNCH(1, 2, 2); else TF_JK_LAUNCH(1, 1, 2);
            } else if (nlc == 2) {
                if (JB == 2) TF_JK_LAUNCH(2, 2, 2); else TF_JK_LAUNCH(2, 1, 2);
            } else
                TF_JK_LAUNCH(4, 1, 2);
        }
#undef TF_JK_LAUNCH
        span.end();
    }
    for (int d = 0; d < nd; ++d)
        hipLaunchKernelGGL(jk_reduce_kernel, dim3(N, (N + 63) / 64), dim3(256), 0, st, A.Jrow + (size_t)d * ctx->n_rows,
                           Kp + (size_t)d * ctx->n_rows * 2 * ld, ctx->d_rowmap, N, ld, dJ[d], dK[d]);
    return TF_OK;
}

// The single exchange step of a sharded Fock build: the partial J and K of nd densities are stacked in one
// staging buffer [2][nd][N][N] and summed over the ranks by the caller's all-reduce (torch.distributed over RCCL in tuna_amd).
static int allreduce_jk(tf_ctx *ctx, int nd, double *const *dJ, double *const *dK, hipStream_t st)
{
    if (ctx->world == 1) return TF_OK;
    if (ctx->comm) {
        // in the library: ncclAllReduce of J and of K where they lie, one group, on the build's stream (no staging copy, no status word: a
        // failed rank fails the collective for every rank)
        const size_t nn1 = (size_t)ctx->N * ctx->N;
        int grc = tfrccl::GroupStart();
        for (int d = 0; d < nd && !grc; ++d) {
            grc = tfrccl::AllReduce(dJ[d], dJ[d], nn1, tfrccl::kFloat64, tfrccl::kSum, ctx->comm, st);
            if (!grc) grc = tfrccl::AllReduce(dK[d], dK[d], nn1, tfrccl::kFloat64, tfrccl::kSum, ctx->comm, st);
        }
        const int erc = tfrccl::GroupEnd();
        if (grc || erc) TF_FAIL(ctx, TF_ENODEVICE, "ncclAllReduce of [J;K] failed: %s", tfrccl::errstr(grc ? grc : erc).c_str());
        return TF_OK;
    }
    if (!ctx->allreduce)
        TF_FAIL(ctx, TF_EINVAL, "the tensor is sharded over %d ranks: attach an RCCL communicator (tf_comm_init) or register the all-reduce of the partial [J;K] with tf_set_allreduce", ctx->world);
    const size_t nn = (size_t)ctx->N * ctx->N, need = 2 * (size_t)nd * nn;
    // one slot beyond the payload carries a status word through the same collective: a rank whose exchange step failed locally (the
    // hook sets it) makes the sum non-zero on EVERY rank, so that all of them return an error instead of some waiting in a collective
    HIPCHK(ctx, (hipError_t)ctx->blk.ensure(CB_JKSTAGE, (need + 1) * sizeof(double)));
    for (int d = 0; d < nd; ++d) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_jkstage() + (size_t)d * nn, dJ[d], nn * sizeof(double), hipMemcpyDeviceToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_jkstage() + (size_t)(nd + d) * nn, dK[d], nn * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    HIPCHK(ctx, hipMemsetAsync(ctx->d_jkstage() + need, 0, sizeof(double), st));
    const int rc = ctx->allreduce(ctx->allreduce_user, ctx->d_jkstage(), (int64_t)(need + 1), (void *)st);
    if (rc) TF_FAIL(ctx, TF_ENODEVICE, "the registered all-reduce failed (code %d)", rc);
    double status = 0.0;
    HIPCHK(ctx, hipMemcpyAsync(&status, ctx->d_jkstage() + need, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (status != 0.0) TF_FAIL(ctx, TF_ENODEVICE, "the exchange step of the sharded Fock build failed on %g rank(s): every rank stops", status);
    for (int d = 0; d < nd; ++d) {
        HIPCHK(ctx, hipMemcpyAsync(dJ[d], ctx->d_jkstage() + (size_t)d * nn, nn * sizeof(double), hipMemcpyDeviceToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(dK[d], ctx->d_jkstage() + (size_t)(nd + d) * nn, nn * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    return TF_OK;
}

int tf_fock_jk_device(tf_ctx *ctx, int n_dens, const double *dP, double *dJ, double *dK, void *stream)
{
    if (!ctx) return TF_EINVAL;
    if (!ctx->have_eri) TF_FAIL(ctx, TF_EINVAL, "tf_fock_jk: call tf_build_eri first");
    if (n_dens < 1 || !dP || !dJ || !dK) TF_FAIL(ctx, TF_EINVAL, "tf_fock_jk: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)ctx->N * ctx->N;
    const int chunk = ctx->layout == 2 ? 8 : 2;                  // densities per pass over the tensor: two (packed / rows), up to eight (tiles)
    for (int d = 0; d < n_dens; d += chunk) {
        const int nd = std::min(chunk, n_dens - d);
        const JkSlots s(nd, nn, dP + d * nn, dJ + d * nn, dK + d * nn);
        int rc = launch_jk(ctx, nd, s.p, s.j, s.k, (hipStream_t)stream);
        if (rc) return rc;
        if (ctx->comm && ctx->world > 1 && (rc = allreduce_jk(ctx, nd, s.j, s.k, (hipStream_t)stream))) return rc;   // in the library, on the same stream
    }
    return TF_OK;
}

int tf_fock_jk(tf_ctx *ctx, int n_dens, const double *P, double *J, double *K)
{
    if (!ctx) return TF_EINVAL;
    if (!ctx->have_eri) TF_FAIL(ctx, TF_EINVAL, "tf_fock_jk: call tf_build_eri first");
    if (n_dens < 1 || !P || !J || !K) TF_FAIL(ctx, TF_EINVAL, "tf_fock_jk: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)ctx->N * ctx->N;
    const int chunk = ctx->layout == 2 ? 8 : 2;
    const tf_ctx::JkAll &A = ctx->jk.all;
    for (int d = 0; d < n_dens; d += chunk) {
        const int nd = std::min(chunk, n_dens - d);
        HIPCHK(ctx, hipMemcpy(A.P, P + d * nn, nd * nn * sizeof(double), hipMemcpyHostToDevice));
        const JkSlots s(nd, nn, A.P, A.J, A.K);
        int nonsym[8] = {0, 0, 0, 0, 0, 0, 0, 0};                // the packed / tiles layouts need a second pass for a non-symmetric density
        const int N = ctx->N;
        for (int q = 0; q < nd; ++q) {
            const double *Pq = P + (d + q) * nn;
            for (int a = 0; a < N && !nonsym[q]; ++a)
                for (int b = 0; b < a; ++b)
                    if (Pq[(size_t)a * N + b] != Pq[(size_t)b * N + a]) { nonsym[q] = 1; break; }
        }
        int rc = launch_jk(ctx, nd, s.p, s.j, s.k, 0, nonsym);
        if (rc) return rc;
        if (ctx->comm && ctx->world > 1 && (rc = allreduce_jk(ctx, nd, s.j, s.k, 0))) return rc;     // a communicator is attached: the sums over the ranks
        HIPCHK(ctx, hipMemcpy(J + d * nn, A.J, nd * nn * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(K + d * nn, A.K, nd * nn * sizeof(double), hipMemcpyDeviceToHost));
    }
    HIPCHK(ctx, hipGetLastError());
    return TF_OK;
}

int tf_jk_profile(tf_ctx *ctx, int enable)
{
    if (!ctx) return TF_EINVAL;
    ctx->prof_jk = enable != 0;
    ctx->prof.used = 0;
    return TF_OK;
}

int tf_jk_profile_read(tf_ctx *ctx, double *seconds_total, int64_t *launches)
{
    if (!ctx || !seconds_total || !launches) return TF_EINVAL;
    double tot = 0.0;
    for (size_t k = 0; k + 1 < ctx->prof.used; k += 2) {
        HIPCHK(ctx, hipEventSynchronize(ctx->prof.ev[k + 1]));
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->prof.ev[k], ctx->prof.ev[k + 1]));
        tot += ms * 1e-3;
    }
    *seconds_total = tot;
    *launches = (int64_t)(ctx->prof.used / 2);
    ctx->prof.used = 0;
    return TF_OK;
}

// Debug / test aid: copies of the partial-sum buffers of the last packed J/K pass and of its group table (one density):
// which = 0 DIc [groups][N], 1 DIr [groups][RS], 2 DJc [rows][N], 3 DJr [rows][RS]; returns the number of doubles copied (<= n) or < 0.
long long tf_debug_partials(tf_ctx *ctx, int which, double *host, long long n)
{
    if (!ctx || !ctx->have_eri || ctx->layout != 1 || !host) return TF_EINVAL;
    const tf_ctx::JKTables &T = ctx->jk.packed.t[0];
    const size_t ng = (size_t)std::max(1, T.n_groups), nrows = (size_t)std::max<long long>(1, ctx->n_rows), N = (size_t)ctx->N, RS = (size_t)ctx->bl.RS;
    const double *src = nullptr; size_t cnt = 0;
    switch (which) {
    case 0: src = ctx->jk.packed.DI; cnt = ng * N; break;
    case 1: src = ctx->jk.packed.DI + ng * N; cnt = ng * RS; break;
    case 2: src = ctx->jk.packed.DJ; cnt = nrows * N; break;
    case 3: src = ctx->jk.packed.DJ + nrows * N; cnt = nrows * RS; break;
    case 4: src = ctx->jk.packed.D; cnt = N * N; break;
    default: return TF_EINVAL;
    }
    cnt = std::min<size_t>(cnt, (size_t)n);
    if (hipMemcpy(host, src, cnt * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return TF_ENODEVICE;
    return (long long)cnt;
}
// group table of the one-density pass: per group {i, j0, nr, r0, c} (internal indices); returns the number of groups
int tf_debug_groups(tf_ctx *ctx, int32_t *out5, int max_groups)
{
    if (!ctx || !ctx->have_eri || ctx->layout != 1) return TF_EINVAL;
    const tf_ctx::JKTables &T = ctx->jk.packed.t[0];
    std::vector<JKGroup> g((size_t)T.n_groups);
    if (T.n_groups && hipMemcpy(g.data(), T.d_groups, g.size() * sizeof(JKGroup), hipMemcpyDeviceToHost) != hipSuccess) return TF_ENODEVICE;
    for (int k = 0; k < T.n_groups && k < max_groups; ++k) { out5[5 * k] = g[k].i; out5[5 * k + 1] = g[k].j0; out5[5 * k + 2] = g[k].nr; out5[5 * k + 3] = g[k].r0; out5[5 * k + 4] = g[k].c; }
    return T.n_groups;
}
