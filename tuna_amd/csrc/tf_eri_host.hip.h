// tf_eri_host.hip.h -- host side of the tensor build: the knobs, the plan of one build (struct EriBuild), its units,
// tf_build_eri and the small tensor queries.  Included by tf_device.hip inside its extern "C" block, one translation unit: tf_ctx,
// DeviceBlocks, tf_malloc, upload and free_eri are defined in tf_ctx.hip.h, build_blocked_layout in tf_basis_host.hip.h, the shard planners
// in tf_shard_plan.h, all above this include.  No kernel is in here; the
// LDS carve-outs and the team-size choice are the pure functions of tf_eri_plan.h.

// AO-level CSR of U (or identity for Cartesian output) on the device
static int upload_csr(tf_ctx *ctx, int spherical)
{
    const tf::Basis &bs = ctx->bs;
    std::vector<int> ptr{0}, idx;
    std::vector<double> val;
    if (spherical) {
        std::vector<double> blk;
        for (const auto &sh : bs.shells) {
            tf::sph_block(sh.L, blk);
            for (int r = 0; r < sh.nsph; ++r) {
                for (int c = 0; c < sh.ncomp; ++c) {
                    const double v = blk[(size_t)r * sh.ncomp + c];
                    if (v != 0.0) { idx.push_back(sh.cart_off + c); val.push_back(v); }
                }
                ptr.push_back((int)idx.size());
            }
        }
    } else {
        for (int i = 0; i < bs.n_cart; ++i) { idx.push_back(i); val.push_back(1.0); ptr.push_back(i + 1); }
    }
    int rc;
    if ((rc = upload(ctx, ptr, CB_CSR_PTR)) || (rc = upload(ctx, idx, CB_CSR_IDX)) || (rc = upload(ctx, val, CB_CSR_VAL))) return rc;
    return TF_OK;
}

// work tables of the J/K kernel for groups of RB rows (8: one density per pass; 4: two), built by tf_packed_host.h
static int upload_jk_tables(tf_ctx *ctx, const tfp::RowTables &rows, int RB, tf_ctx::JKTables &T)
{
    const tfp::HostLayout &H = ctx->hl;
    tfp::JKWork W;
    tfp::build_jk_work(H, rows, RB, W);
    if (g_dbg) {
        long long st_all = 0, st_cd = 0;                       // wave steps of the two lists (what a pass costs)
        for (const JKTask &t : W.tasks) {
            const JKSuper &sg = W.supers[t.super];
            const long long stp = (long long)tfp::task_steps(H, sg, t) * ((sg.ng + TF_JKP_GPW - 1) / TF_JKP_GPW);
            st_all += stp;
            if (tfp::task_class_diagonal(H, sg, t)) st_cd += stp;
        }
        DBG("J/K tasks: %zu (class-diagonal list: %zu), wave steps %lld (%lld)", W.tasks.size(), W.tasks_cd.size(), st_all, st_cd);
    }
    int rc2;
    DeviceBlocks &mem = ctx->build_mem;
    if ((rc2 = upload(ctx, W.groups, &T.d_groups, mem)) || (rc2 = upload(ctx, W.gfirst, &T.d_gfirst, mem)) ||
        (rc2 = upload(ctx, W.tasks, &T.d_tasks, mem)) || (rc2 = upload(ctx, W.supers, &T.d_supers, mem)) ||
        (rc2 = upload(ctx, W.tasks_cd, &T.d_tasks_cd, mem)))
        return rc2;
    T.n_groups = (int)W.groups.size(); T.n_tasks = (int)W.tasks.size(); T.n_supers = (int)W.supers.size();
    T.n_tasks_cd = (int)W.tasks_cd.size();
    std::copy(W.bucket, W.bucket + 4, T.bucket); std::copy(W.bucket_cd, W.bucket_cd + 4, T.bucket_cd);
    T.nseg = W.nseg;
    T.ypart_len = W.ypart_len;
    T.jp = W.jp;
    return TF_OK;
}

// the device reads (i, j) pairs as int2
static_assert(sizeof(TFInt2) == sizeof(int2) && offsetof(TFInt2, y) == offsetof(int2, y), "TFInt2 must have the layout of int2");
static int upload_int2(tf_ctx *ctx, const std::vector<TFInt2> &h, int2 **d) { return upload(ctx, h, reinterpret_cast<TFInt2 **>(d), ctx->build_mem); }

static double seconds_between(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, a, b);
    return ms * 1e-3;
}

extern "C++" {
// ---- environment knobs of the tensor build: what they do, default, WHEN they are read, who uses them -------------------------------
// per build (read once at the start of tf_build_eri into EriKnobs; tests set them in a running process):
// TF_ERI_MODE           "c..": per-class launches, else the small-problem mode.  By size.  test_gpu_eri_shapes, test_gpu_parity, test_gpu_sharded, gpu_eri_ab
// TF_SLAB_MB            slab size in MiB (>= 1).  1-4 GiB by size.  test_gpu_eri_shapes (tests/eri_shapes.py)
// TF_SLAB_ROWS          slab cut in Cartesian bra rows (1: one bra shell pair per slab).  Unset.  test_gpu_eri_shapes, gpu_eri_ab
// TF_ERI_LAYOUT         "t" tiles, "p" packed, "r" rows: overrides tf_set_eri_layout.  Unset.  gpu_tiles_perf, gpu_field_timing
// TF_ERI_NSTREAM        streams the launches of a slab are spread over (1 .. 8).  8.  test_gpu_eri_shapes
// TF_ERI_NQ             small-problem mode: streams the group launches are balanced over.  max(4, min(8, GPU_MAX_HW_QUEUES)).  test_gpu_eri_shapes
// GPU_MAX_HW_QUEUES     the HIP runtime's own variable, only READ here (the default of TF_ERI_NQ); the library never sets it
// TF_ERI_FAMILIES       "0" / other: ket families off / on.  By primitive quartets (>= 8e6).  test_gpu_eri_shapes, test_gpu_parity, gpu_eri_ab
// TF_ERI_CC_FAMILIES    "0": no families on both sides of contracted-contracted launches.  On.  test_gpu_eri_shapes, test_gpu_parity
// TF_ERI_BRA_FAMILIES   "1": bra families against uncontracted kets.  Off.  test_gpu_eri_shapes, test_gpu_parity, gpu_eri_ab
// TF_ERI_DBG_NPQ        lo:hi -- eri_cfact_kernel computes only quartets with so many primitive quartets (profiling aid).  All.  tools/README.md
// TF_ERI_NOFACT         set: eri_class_kernel instead of eri_fact_kernel.  Unset.  test_gpu_eri_shapes, gpu_eri_ab
// once per process (function-local static of the accessor, called where the knob is used: the first use reads it; tests set them in
// child processes):
// TF_ERI_TEAM           "0": no team kernels.  On.  First build.  test_gpu_eri_shapes, gpu_eri_ab
// TF_ERI_TEAMC          "1": eri_teamc_kernel in the small-problem mode.  Off.  First build.  test_gpu_eri_shapes, gpu_eri_ab
// TF_TEAMC_PQMAX        most primitive quartets of a quartet eri_teamc_kernel takes.  700.  First build.  test_gpu_eri_shapes
// TF_ERI_TEAM_SIZE      16 / 64 / 256: forced team size where instantiated and fitting.  0.  First team-eligible class launch.  test_gpu_eri_shapes
// TF_TEAM_LDS_KB        soft LDS limit of the 64-lane teams, KB.  76.  As above.  test_gpu_eri_shapes
// TF_TEAM16_NNZ         most parity-allowed components of a 16-lane class.  96.  As above.  test_gpu_eri_shapes
// TF_TEAM_KPW_DIV, TF_TEAM_KPW_MAX   ket groups per workgroup: launch size aimed at, most groups.  2048, 16.  As above.  test_gpu_eri_shapes
// TF_ERI_FACT_THREADS   64 / 128: smaller workgroups of eri_fact_kernel.  256.  First eri_fact_kernel launch.  gpu_eri_ab
// TF_CF_NBT, TF_CF_XZ, TF_CF_E   eri_cfact_kernel: batch aimed at, X / Z doubles, staged Hermite doubles.  24, 768, 1024.  First small-problem build.  tools/README.md
// TF_ERI_GENERIC_OLD    set: the component-per-lane kernel for every group launch.  Unset.  First small-problem slab.  test_gpu_eri_shapes, gpu_eri_ab
// TF_ERI_CLASS_TIMES    set: every class launch alone on the device, timed and printed.  Unset.  First class launch.  gpu_eri_classes
// TF_TILE_PART_STEPS, TF_TILE_KSUB   tiles: steps per part of the stored task list; strip height of the one-density list (16, 32, 64).
//                       TT_STEPS_MAX, 32.  First tiles build.  gpu_tiles_perf, test_gpu_fock_shapes
struct EriKnobs {
    static int env_int(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }
    static bool env_is(const char *name, char c) { const char *e = getenv(name); return e && e[0] == c; }
    // per build
    int mode = getenv("TF_ERI_MODE") ? env_is("TF_ERI_MODE", 'c') : -1;                       // -1 unset, 1 per class, 0 small-problem mode
    int slab_mb = getenv("TF_SLAB_MB") ? std::max(1, env_int("TF_SLAB_MB", 1)) : 0;           // 0 unset
    long long slab_rows = getenv("TF_SLAB_ROWS") ? std::max<long long>(1, atoll(getenv("TF_SLAB_ROWS"))) : 0;   // 0 unset
    char layout = getenv("TF_ERI_LAYOUT") ? getenv("TF_ERI_LAYOUT")[0] : 0;                   // 0 unset
    int families = getenv("TF_ERI_FAMILIES") ? !env_is("TF_ERI_FAMILIES", '0') : -1;          // -1 unset, 0 off, 1 on
    bool cc_fam_off = env_is("TF_ERI_CC_FAMILIES", '0'), bra_fam = env_is("TF_ERI_BRA_FAMILIES", '1'), nofact = getenv("TF_ERI_NOFACT") != nullptr;
    int nstream = std::max(1, std::min((int)tf_ctx::NSTREAM_MAX, env_int("TF_ERI_NSTREAM", tf_ctx::NSTREAM_MAX)));
    // (as many streams as the process has hardware queues: 4 unless GPU_MAX_HW_QUEUES says otherwise -- tuna_amd sets 16)
    int nq = getenv("TF_ERI_NQ") ? std::max(1, env_int("TF_ERI_NQ", 1)) : std::max(4, std::min(8, std::max(1, env_int("GPU_MAX_HW_QUEUES", 4))));
    int dbg_npq_lo = 0, dbg_npq_hi = 0x7fffffff;
    EriKnobs() { if (const char *e = getenv("TF_ERI_DBG_NPQ")) (void)sscanf(e, "%d:%d", &dbg_npq_lo, &dbg_npq_hi); }
    // once per process
    static bool team_off() { static const bool v = env_is("TF_ERI_TEAM", '0'); return v; }
    static bool teamc_on() { static const bool v = env_is("TF_ERI_TEAMC", '1'); return v; }
    static int teamc_pqmax() { static const int v = env_int("TF_TEAMC_PQMAX", 700); return v; }
    static int team_size() { static const int v = env_int("TF_ERI_TEAM_SIZE", 0); return v; }
    static int team_lds_kb() { static const int v = env_int("TF_TEAM_LDS_KB", 76); return v; }
    static int team16_nnz() { static const int v = env_int("TF_TEAM16_NNZ", 96); return v; }
    static long long team_kpw_div() { static const long long v = getenv("TF_TEAM_KPW_DIV") ? atoll(getenv("TF_TEAM_KPW_DIV")) : 2048; return v; }
    static long long team_kpw_max() { static const long long v = getenv("TF_TEAM_KPW_MAX") ? atoll(getenv("TF_TEAM_KPW_MAX")) : 16; return v; }
    // (TF_ERI_FACT_THREADS=64|128: smaller workgroups for experiments -- measured slower at N = 400, 127 / 159 ms against 113-127 ms:
    // the LDS of a quartet limits the workgroups per CU, so fewer waves per workgroup are fewer waves per CU)
    static int fact_threads() { static const int v = env_int("TF_ERI_FACT_THREADS", 0); return (v == 64 || v == 128) ? v : TF_ERI_THREADS; }
    static tfe::CFKnobs cfact() { static const tfe::CFKnobs v{env_int("TF_CF_NBT", 24), env_int("TF_CF_XZ", 768), env_int("TF_CF_E", 1024)}; return v; }
    static bool generic_old() { static const bool v = getenv("TF_ERI_GENERIC_OLD") != nullptr; return v; }
    static bool class_times() { static const bool v = getenv("TF_ERI_CLASS_TIMES") != nullptr; return v; }
    static int tile_part_steps() { static const int v = std::min(TT_STEPS_MAX, getenv("TF_TILE_PART_STEPS") ? std::max(1, atoi(getenv("TF_TILE_PART_STEPS"))) : TT_STEPS_MAX); return v; }
    static int tile_ksub() { static const int v = env_int("TF_TILE_KSUB", 32); return v; }     // (measured at N = 400: strips of 32 rows 2.2 ms, of 64 3.0, of 16 2.3)
};

// ---- the tensor build: tf_build_eri is a short sequence of units over one plan -----------------------------
// The device lists and timing events that live for ONE build; the lists are held by a DeviceBlocks.  release() is what the end of a
// successful build does (the device is drained by then); the destructor covers every other way out: launches may still be in flight,
// so it drains the device first.
struct EriBuildMem {
    tf_ctx *ctx;
    DeviceBlocks blocks;
    std::vector<hipEvent_t> events;
    explicit EriBuildMem(tf_ctx *c) : ctx(c) {}
    template <class T> int alloc(T **p, size_t bytes) { HIPCHK(ctx, blocks.take((void **)p, bytes)); return TF_OK; }
    template <class T> int up(const std::vector<T> &h, T **d) { *d = nullptr; return upload(ctx, h, d, blocks); }
    int event(hipEvent_t *e)
    {
        HIPCHK(ctx, hipEventCreate(e));
        events.push_back(*e);
        return TF_OK;
    }
    void release()
    {
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        events.clear(); blocks.clear();
    }
    ~EriBuildMem()
    {
        if (blocks.held.empty() && events.empty()) return;
        (void)hipDeviceSynchronize();
        release();
    }
};

// TF_ERI_CLASS_TIMES=1 (diagnostic): every class launch alone on the device, its time printed with the class
struct ClassTimer {
    bool on; const QClass &q; unsigned nb; std::chrono::steady_clock::time_point t0;
    ClassTimer(bool o, const QClass &qq, unsigned n) : on(o), q(qq), nb(n) { if (on) { (void)hipDeviceSynchronize(); t0 = std::chrono::steady_clock::now(); } }
    ~ClassTimer() {
        if (!on) return;
        (void)hipDeviceSynchronize();
        const double ms = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "[tf eri class] (%d %d|%d %d) npq %d bra %u ket %d quartets %.0f: %.3f ms, %.1f ns per quartet\n", q.La, q.Lb, q.Lc, q.Ld,
                q.npq, nb, q.n_ket, (double)nb * q.n_ket, ms, 1e6 * ms / ((double)nb * q.n_ket));
    }
};

// The plan of one build: what the units below share.  plan_storage and plan_generation fill it, run_slab walks it.
struct EriBuild {
    tf_ctx *ctx;
    const tf::Basis &bs;
    const tfp::HostLayout &H;
    const int spherical;
    const EriKnobs knobs;                                       // the per-build knobs, read here: at the start of the build
    EriBuildMem mem;
    EriBuild(tf_ctx *c, int sph) : ctx(c), bs(c->bs), H(c->hl), spherical(sph), mem(c) {}

    static constexpr int NLPG = 7, NGRP = 2 * NLPG;
    static constexpr int FAM_MM = 9, FAM_MA_CC = 3;
    struct KClassTab { int pS[5] = {0, 0, 0, 0, 0}; int nkap = 0, nnzT = 0, tp_off = 0, te_off = 0; };
    struct BraFam { int *d_ptr = nullptr, *d_mem = nullptr; unsigned n = 0; };
    typedef std::map<std::pair<size_t, int>, BraFam> BraFams;  // by (first position of the run of bra pairs, largest family)
    struct TcLaunch { int LAB, LCD, team; size_t lds; std::vector<TeamTask> tasks; std::vector<double> cost; };

    // The members, grouped by the stage that fills them (plain structs: no accessors)
    struct Storage {                                            // plan_storage (nsh: plan_work_counters, ncls: plan_ket_lists)
        int Nc = 0, N = 0, ld = 0, npairs = 0, nsh = 0, ncls = 0;
        bool packed = false, tiles = false;
        long long row_len = 0;
        std::vector<long long> pair_rows;
        std::vector<int> owner;
        tfp::RowTables rows;
    } sto;
    struct Slab {                                               // plan_slab_size, plan_work_counters; the counters run_slab adds to
        bool per_class = false;
        double *d_C = nullptr, *d_T2 = nullptr;
        long long max_rows_c = 1, cut_rows = 1;                 // rows the slab buffers hold; rows at which run_slab cuts (<= max_rows_c)
        double t_stage[4] = {0, 0, 0, 0};
        long long n_quart = 0, n_primq = 0, n_compq = 0;
        std::vector<long long> cum_pairs, cum_pp, cum_comp;
        std::vector<std::array<double, 4>> pairW, pairNc, cumW;
        std::vector<std::array<double, 44>> cumNL;
        double nominal_flops = 0.0;
        std::chrono::steady_clock::time_point t_wall0;
    } slab;
    struct Kets {                                               // plan_ket_lists, plan_ket_families; mine_sorted: plan_generation
        std::vector<int> ket_sorted, ket_off, cls_maxnpp;
        int kets_goff[NGRP + 1] = {};
        int *d_kets = nullptr, *d_kets_all = nullptr;
        std::vector<int> kets_all_host;                          // same order as d_kets_all
        bool fam_off = false, bra_fam_on = false, fam_any = false;
        int fam_goff[NGRP + 1] = {};
        int *d_fam_heads = nullptr, *d_fam_ptr = nullptr, *d_fam_mem = nullptr;
        std::vector<int> psid;
        std::vector<int> mine_sorted;
    } kets;
    struct Run {                                                // setup_streams; the counters the launches add to
        int NSTREAM = 1;
        hipStream_t *streams = nullptr;
        hipEvent_t *sev = nullptr;
        int launch_count = 0;
        long long stats[TF_ERI_STAT_COUNT] = {};               // host counters of tf_eri_build_stats: incremented where the launches are made
    } run;
    void count(int family) { ++run.stats[family]; ++run.stats[TF_ERI_STAT_LAUNCHES]; }
    struct LaunchTables {                                       // plan_generation, make_caps, make_lrecs
        std::vector<LRec> lrecs_host;                          // per (La, Lb | Lc, Ld), filled by make_lrecs
        hipError_t team_error = hipSuccess;                    // first failed launch of a team kernel
        bool use_team_pc = false, use_teamc = false, use_team = false;
        int teamc_pqmax = 700;
        CFCaps gcaps[NGRP][NGRP];
        bool gcaps_fit[NGRP][NGRP], gcaps_gtab[NGRP][NGRP];
    } lt;
    struct TeamTables {                                         // plan_team_tables; d_brarec, d_bra_base: per slab (run_slab)
        std::vector<KClassTab> kct;
        int *d_kcnt = nullptr;
        KetRec *d_ketrec = nullptr;                            // parallel to d_kets (class-sorted ket list)
        std::vector<int> flat_off;
        BraRec *d_brarec = nullptr;                            // parallel to the slab's bra list d_bra
        const int *d_bra_base = nullptr;
    } tt;
    struct IndexLists {                                         // plan_index_buffers: the slabs' index lists (two sets) and timing events
        size_t cap_bra = 0, cap_out = 0, out_bytes = 0, rowcls_bytes = 0;
        int *d_bra = nullptr, *d_bra_alloc = nullptr;
        long long *d_braoff = nullptr, *d_braoff_alloc = nullptr;
        void *d_out = nullptr, *d_out_alloc = nullptr;
        BraRec *d_brarec_alloc = nullptr;
        signed char *d_rowcls = nullptr, *d_rowcls_alloc = nullptr;  // parity class of every slab row (small-problem mode, packed layout)
        long long slab_no = 0;
        std::vector<hipEvent_t> tev;                               // 4 timing events per slab, read at the end
        std::vector<hipEvent_t> tev2;                              // 2 per slab around the task-list team kernels (they count as ERI kernels)
        size_t cursor = 0;
    } ix;
    struct Teamc {                                              // small-problem mode with team kernels: teamc_class, teamc_tasks
        std::vector<TClass> tcs_host;
        std::vector<int> tc_of, tc_team;                           // -2: not made yet, -1: not eligible
        std::vector<size_t> tc_lds;
        bool any_wide_pair = false;                                // a pair sum beyond the team kernels' instantiations
        int max_npp_all = 1;
        TClass *d_tcs = nullptr; TeamTask *d_tasks = nullptr;
        size_t d_tcs_cap = 0, d_tasks_cap = 0;
    } tc;

    int out_dim(const tf::Shell &s) const { return spherical ? s.nsph : s.ncomp; }
    int out_off(const tf::Shell &s) const { return spherical ? s.sph_off : s.cart_off; }
    long long pair_cost(int p) const {                             // primitive pairs x components: what a quartet with this pair costs
        return (long long)bs.pairs[p].npp * bs.shells[bs.pairs[p].A].ncomp * bs.shells[bs.pairs[p].B].ncomp;
    }
    // groups of shell pairs: by La + Lb (tfe::lp_group) and by contracted / uncontracted
    int pair_group(int p) const { return 2 * tfe::lp_group(bs.pairs[p].La + bs.pairs[p].Lb) + (bs.pairs[p].npp > 1 ? 1 : 0); }

    int plan_storage();
    int upload_consumer_tables();
    int plan_generation();
    int plan_slab_size();
    void plan_work_counters();
    int plan_ket_lists();
    int plan_ket_families();
    int setup_streams();
    int plan_team_tables();
    void forget_team_tables();
    int plan_index_buffers();
    TClass tclass_common(int bcls, int kcls, int &maxblk, int &maxK, int &nnzc) const;
    void launch_class(int bcls, int kcls, int max_npp_bra, unsigned n_bra, const int *d_bra, const long long *d_braoff, int bra_Amax);
    void launch_generic_old(unsigned n_bra, const int *d_bra, const long long *d_braoff, unsigned n_ket, const int *d_ket, hipStream_t st);
    tfe::GroupStat group_stat(const int *pairs_host, size_t n) const;
    void make_caps();
    int make_lrecs(bool with_caps);
    const BraFam *bra_families(BraFams &bra_fams, const std::vector<int> &bra_host, size_t b0, size_t b1, int most);
    int launch_generic(const std::vector<int> &bra_host, const int *d_bra, const long long *d_braoff);
    int teamc_class(int bcls, int kcls);
    int teamc_tasks(const std::vector<int> &bra, const std::vector<long long> &braoff, std::vector<TcLaunch> &tcl, bool &old_needed);
    int launch_teamc(const std::vector<TcLaunch> &tcl);
    int run_slab();
    int finish();
    void abandon();
    int alloc_jk_scratch();
};

// Storage: layout choice, owners of the bra shell pairs, host tables (tf_packed_host.h / tf_tiles_host.h), tensor buffer, table uploads
int EriBuild::plan_storage()
{
    int rc;
    sto.Nc = bs.n_cart; sto.N = spherical ? bs.n_sph : bs.n_cart; sto.ld = (sto.N + 1) & ~1;
    if (ctx->grid.G > 0 && ctx->grid.N != sto.N) tfdft::release(ctx->grid);   // (a grid of the other AO representation)
    ctx->spherical = spherical; ctx->N = sto.N; ctx->ld = sto.ld;
    sto.npairs = (int)bs.pairs.size();

    // ---- which bra shell pairs (= row blocks) belong to this rank: longest-processing-time on row counts
    for (int p = 0; p < sto.npairs; ++p) {
        ctx->host_pairs[p].outoff_a = out_off(bs.shells[bs.pairs[p].A]);
        ctx->host_pairs[p].outoff_b = out_off(bs.shells[bs.pairs[p].B]);
    }
    HIPCHK(ctx, hipMemcpy(ctx->d_pairs, ctx->host_pairs.data(), (size_t)sto.npairs * sizeof(DPair), hipMemcpyHostToDevice));
    // layout: packed (8-fold unique, tf_jkpacked.hip.h) unless asked otherwise
    int layout = ctx->layout_req;
    if (const char e = knobs.layout) layout = (e == 't') ? 2 : ((e == 'p') ? 1 : (e == 'r' ? 0 : layout));
    if (layout < 0) layout = 1;                                       // (tiles: opt-in -- measured slower than packed at N = 400)
    ctx->layout = layout;
    // packed: the symmetry-unique, parity-allowed values (layouts 1 and 2: the generation and its slab are the same); tiles: stored
    // j-innermost in (i, class pair, strip, chunk) regions (tf_tiles.h) instead of row by row (tf_jkpacked.hip.h)
    sto.packed = layout >= 1; sto.tiles = layout == 2;
    sto.pair_rows.assign(sto.npairs, 0);
    for (int p = 0; p < sto.npairs; ++p) {
        const tf::Shell &a = bs.shells[bs.pairs[p].A], &b = bs.shells[bs.pairs[p].B];
        sto.pair_rows[p] = (bs.pairs[p].A == bs.pairs[p].B) ? (long long)out_dim(a) * (out_dim(a) + 1) / 2
                                                        : (long long)out_dim(a) * out_dim(b);
    }
    {
        std::vector<int> dims(bs.shells.size());
        for (size_t q = 0; q < dims.size(); ++q) dims[q] = out_dim(bs.shells[q]);
        shard_plan_pairs(dims, sto.packed, ctx->world, getenv("TF_SHARD_PLAN"), sto.owner);           // pair index A(A+1)/2 + B = position in bs.pairs
    }
    ctx->my_pairs.clear();
    for (int p = 0; p < sto.npairs; ++p)
        if (sto.owner[p] == ctx->rank) ctx->my_pairs.push_back(p);

    // ---- parity classes of the output AOs and the layout tables (packed layout)
    if (sto.packed) {
        std::vector<int> cls;
        tfp::ao_classes(bs, spherical != 0, cls);
        if ((rc = build_blocked_layout(ctx, cls))) return rc;
    }
    // ---- row tables
    {
        std::vector<int> ooff(bs.shells.size()), odim(bs.shells.size());
        for (size_t q = 0; q < odim.size(); ++q) { ooff[q] = out_off(bs.shells[q]); odim[q] = out_dim(bs.shells[q]); }
        tfp::list_rows(bs.pairs, ooff, odim, ctx->my_pairs, sto.N, sto.rows);
    }
    if (sto.packed) tfp::pack_rows(H, sto.tiles, sto.rows);
    const std::vector<TFInt2> &row_ij = sto.rows.row_ij;
    if (sto.packed && !sto.tiles) ctx->n_elems = sto.rows.n_elems;
    if (sto.tiles) {
        // regions of the stored tensor and the task list of the Fock kernel (tf_tiles_host.h)
        const tft::ClassInfo C = tfp::class_info(H);
        std::vector<std::pair<int, int>> rows_ij(row_ij.size());
        for (size_t r = 0; r < row_ij.size(); ++r) rows_ij[r] = {H.sigma[row_ij[r].x], H.sigma[row_ij[r].y]};
        const int part_steps = EriKnobs::tile_part_steps();
        ctx->tclass = C; ctx->trows = rows_ij;
        std::string e = tft::build(C, rows_ij, part_steps, ctx->tiles);
        if (!e.empty()) TF_FAIL(ctx, TF_EINVAL, "%s", e.c_str());
        const int ksub_env = EriKnobs::tile_ksub();
        ctx->ksub1 = (ksub_env == 64 || ksub_env == 16) ? ksub_env : 32;
        if (ctx->ksub1 != TT_KS) {
            e = tft::build_list(C, ctx->tiles, rows_ij, ctx->ksub1, part_steps, ctx->tsub1);
            if (!e.empty()) TF_FAIL(ctx, TF_EINVAL, "%s", e.c_str());
        }
        if (ctx->tiles.max_slice * (long long)part_steps * 8 > 0x7fffffffLL) TF_FAIL(ctx, TF_EINVAL, "tiles layout: a task's region exceeds the 32-bit offsets of the Fock kernel");
        ctx->n_elems = ctx->tiles.n_elems;
        const tft::Tables &TT = ctx->tiles;
        std::vector<int> tab(TVT_LEN, 0);
        for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) tab[TVT_PID + 4 * a + b] = std::max(0, TT.pid[a][b]);
        for (int p2 = 0; p2 < TT.npair; ++p2) { tab[TVT_PA + p2] = TT.pa[p2]; tab[TVT_PB + p2] = TT.pb[p2]; tab[TVT_PMOFF + p2] = TT.pm_off[p2]; tab[TVT_PMPITCH + p2] = TT.pm_pitch[p2]; }
        for (int q = 0; q < 4; ++q) { tab[TVT_CSTART + q] = H.cstart[q]; tab[TVT_CSIZE + q] = H.csize[q]; }
        DeviceBlocks &mem = ctx->build_mem;
        tf_ctx::JkTiles &Z = ctx->jk.tiles;
        TTask *d_regions = nullptr; TPairI *d_pp = nullptr; TRunI *d_rr = nullptr;
        if ((rc = upload(ctx, TT.primary.tasks_by_region, &d_regions, mem)) || (rc = upload(ctx, TT.primary.pairs, &d_pp, mem)) ||
            (rc = upload(ctx, TT.primary.runs, &d_rr, mem)) || (rc = upload(ctx, tab, &Z.tvtab, mem)))
            return rc;
        TView V{};
        V.regions = d_regions; V.prim_pairs = d_pp; V.prim_runs = d_rr; V.edge_base = TT.edge_base; V.N = sto.N; V.pm_len = TT.pm_len; V.tab = Z.tvtab;
        ctx->tv = V;
        Z.tl1.d_pairs = d_pp; Z.tl1.d_runs = d_rr;
    }
    ctx->n_rows = (long long)row_ij.size();
    sto.row_len = (long long)sto.N * sto.ld;
    if (!sto.packed) ctx->n_elems = ctx->n_rows * sto.row_len;
    if (ctx->n_rows > 0x7fffffffLL) TF_FAIL(ctx, TF_EINVAL, "too many tensor rows for this build");
    {
        // the tensor buffer is kept across builds (geometry scans rebuild a tensor of the same size); it is replaced when it is
        // too small or more than twice too large
#ifdef TF_ABL_ALLVALID
        const size_t need = std::max<size_t>(1, (size_t)ctx->n_elems * sizeof(double)) + (4u << 20);
#else
        const size_t need = std::max<size_t>(1, (size_t)ctx->n_elems * sizeof(double));
#endif
        if (ctx->blk.cap[CB_ERI] > 2 * need + (64u << 20)) ctx->blk.drop(CB_ERI);
        HIPCHK(ctx, (hipError_t)ctx->blk.ensure(CB_ERI, need));
    }
    if ((rc = upload_int2(ctx, row_ij, &ctx->d_row_ij)) || (rc = upload(ctx, sto.rows.rowmap, &ctx->d_rowmap, ctx->build_mem))) return rc;
    if (sto.packed) {
        if (!sto.tiles && ((rc = upload(ctx, sto.rows.rowoff, &ctx->d_rowoff, ctx->build_mem)) || (rc = upload(ctx, sto.rows.rowsec, &ctx->d_rowsec, ctx->build_mem)))) return rc;
        ctx->db.bl = ctx->bl;
        ctx->db.RLS = H.RLS;
    }
    if (sto.tiles) HIPCHK(ctx, hipMemsetAsync(ctx->d_eri(), 0, (size_t)ctx->n_elems * sizeof(double), 0));   // the pad slots of the rows and pieces stay zero
    return TF_OK;
}

// The tables only the CONSUMERS of the tensor need (work tables of the J/K kernel, reduction lists, rows by class) are built on the
// host while the generation kernels run: called behind the launches of the last slab (7 ms of host time at N = 400).
int EriBuild::upload_consumer_tables()
{
    if (!sto.packed) return TF_OK;
    int rc2;
    tfp::ConsumerTables CT;
    tfp::build_class_rows(H, sto.rows, CT);
    std::copy(CT.class_row_off, CT.class_row_off + 5, ctx->class_row_off);
    DeviceBlocks &mem = ctx->build_mem;
    if ((rc2 = upload(ctx, CT.class_rows, &ctx->d_class_rows, mem)) || (rc2 = upload(ctx, CT.row_pos, &ctx->d_row_pos, mem))) return rc2;
    if (sto.tiles) {
        const tft::Tables &TT = ctx->tiles;
        const tft::TaskList &TL = ctx->ksub1 == TT_KS ? TT.primary : ctx->tsub1;
        tf_ctx::JkTiles &Z = ctx->jk.tiles;
        if ((rc2 = tile_list_upload(ctx, TL, ctx->ksub1 != TT_KS, Z.tl1)) || (rc2 = upload(ctx, TT.jlist_ptr, &Z.jlist_ptr, mem)) ||
            (rc2 = upload(ctx, TT.jlist, &Z.jlist, mem)))
            return rc2;
        return TF_OK;
    }
    tf_ctx::JkPacked &K = ctx->jk.packed;
    if ((rc2 = upload_jk_tables(ctx, sto.rows, JKShape<1>::RB, K.t[0])) || (rc2 = upload_jk_tables(ctx, sto.rows, JKShape<2>::RB, K.t[1]))) return rc2;
    tfp::build_reduction_lists(H, sto.rows, CT);
    if ((rc2 = upload(ctx, CT.jptr, &K.jptr, mem)) || (rc2 = upload_int2(ctx, CT.jrows, &K.jrows))) return rc2;
    if ((rc2 = upload(ctx, CT.xorder, &K.xorder, mem))) return rc2;
    return TF_OK;
}

// ---- slabs of bra pairs: Cartesian block -> ket transform -> bra transform -> tensor rows
int EriBuild::plan_slab_size()
{
    int rc;
    // Large problems launch per (bra class, ket class) with the ket transform fused into the ERI kernels: no Cartesian slab at all.
    slab.per_class = (long long)ctx->my_pairs.size() * sto.npairs >= 2000000LL;
    if (knobs.mode >= 0) slab.per_class = knobs.mode == 1;
    // A slab row is one Cartesian bra component pair: Nc^2 Cartesian ket values (small-problem mode only) and the ket-transformed
    // row -- N x ld (rows layout) or the complete-row shape of the packed layout (RLS doubles, ~ N^2 / 8).  1 GiB of slab, more (up
    // to 4 GiB) for big tensors: fewer, larger class launches.
    const size_t cart_row_bytes = (size_t)sto.Nc * sto.Nc * sizeof(double);
    const size_t t2_row_bytes = (sto.packed ? (size_t)H.RLS : (size_t)sto.N * sto.ld) * sizeof(double);
    const size_t slab_row_bytes = std::max<size_t>(8, std::max(t2_row_bytes, slab.per_class ? (size_t)0 : cart_row_bytes));
    size_t slab_total = 0;                                       // this rank's bra rows: one slab if that is <= 4 GiB
    for (int p : ctx->my_pairs) slab_total += (size_t)bs.shells[bs.pairs[p].A].ncomp * bs.shells[bs.pairs[p].B].ncomp * slab_row_bytes;
    size_t slab_bytes = std::min<size_t>((size_t)4 << 30, std::max<size_t>((size_t)1 << 30, std::max((size_t)ctx->n_elems, slab_total)));
    if (knobs.slab_mb) slab_bytes = (size_t)knobs.slab_mb << 20;
    slab.max_rows_c = std::max<long long>(1, (long long)(slab_bytes / slab_row_bytes));
    // TF_SLAB_ROWS=n: the slab in Cartesian bra rows (the 1 MiB floor of TF_SLAB_MB cannot cut a small basis); n = 1 gives one bra
    // shell pair per slab, the finest cut there is
    slab.cut_rows = 0;
    if (knobs.slab_rows) slab.max_rows_c = slab.cut_rows = knobs.slab_rows;
    long long biggest = 1;
    for (int p : ctx->my_pairs)
        biggest = std::max<long long>(biggest, (long long)bs.shells[bs.pairs[p].A].ncomp * bs.shells[bs.pairs[p].B].ncomp);
    slab.max_rows_c = std::max(slab.max_rows_c, biggest);
    {
        long long need = 0;                                      // never more than this rank's rows need
        for (int p : ctx->my_pairs) need += (long long)bs.shells[bs.pairs[p].A].ncomp * bs.shells[bs.pairs[p].B].ncomp;
        slab.max_rows_c = std::max<long long>(biggest, std::min(slab.max_rows_c, need));
    }
    // the buffers hold the largest pair; the cut itself stays at what TF_SLAB_ROWS asked for (a slab always takes its first pair whole)
    slab.cut_rows = slab.cut_rows ? std::min(slab.cut_rows, slab.max_rows_c) : slab.max_rows_c;
    if ((rc = ensure_scratch(ctx, 0, slab.per_class ? 8 : (size_t)slab.max_rows_c * cart_row_bytes)) ||
        (rc = ensure_scratch(ctx, 2, (size_t)slab.max_rows_c * t2_row_bytes)))
        return rc;
    slab.d_C = ctx->scr(0); slab.d_T2 = ctx->scr(2);
    return TF_OK;
}

void EriBuild::plan_work_counters()
{
    // work counters: ket pairs / primitive pairs / component pairs with first shell <= A (the pair list is A-major).  The packed
    // layout computes exactly the kets whose first shell does not exceed the bra's; the rows layout all of them.
    sto.nsh = (int)bs.shells.size();
    slab.cum_pairs.assign(sto.nsh + 1, 0); slab.cum_pp.assign(sto.nsh + 1, 0); slab.cum_comp.assign(sto.nsh + 1, 0);
    for (int p = 0; p < sto.npairs; ++p) {
        const int A = bs.pairs[p].A;
        slab.cum_pairs[A + 1] += 1;
        slab.cum_pp[A + 1] += bs.pairs[p].npp;
        slab.cum_comp[A + 1] += (long long)bs.shells[A].ncomp * bs.shells[bs.pairs[p].B].ncomp;
    }
    for (int a = 0; a < sto.nsh; ++a) { slab.cum_pairs[a + 1] += slab.cum_pairs[a]; slab.cum_pp[a + 1] += slab.cum_pp[a]; slab.cum_comp[a + 1] += slab.cum_comp[a]; }
    // Nominal operation count of the reference algorithm for the quartets this build evaluates: per primitive
    // AO quartet that passes the parity test (pyx:1324-1327), 8 x the inner terms of the loop nest pyx:1179-1217 -- (lx12/2+1)(lx34/2+1)
    // (ly12/2+1)(ly34/2+1)(lz12+1)(lz34+1), a product of a bra and a ket factor -- plus the Boys / R table cost 6 (L+1) + 3 (L+1)^2 / 2 + 60.
    // Per shell pair and parity class c: W = sum of its factor over the component pairs of the class, n = their number.
    slab.pairW.resize(sto.npairs); slab.pairNc.resize(sto.npairs);
    for (int p = 0; p < sto.npairs; ++p) {
        const tf::Shell &sa = bs.shells[bs.pairs[p].A], &sb = bs.shells[bs.pairs[p].B];
        slab.pairW[p] = {0, 0, 0, 0}; slab.pairNc[p] = {0, 0, 0, 0};
        for (int ca = 0; ca < sa.ncomp; ++ca)
            for (int cb = 0; cb < sb.ncomp; ++cb) {
                const int u = sa.comp_off + ca, v = sb.comp_off + cb;
                const int lx = bs.c_lx[u] + bs.c_lx[v], ly = bs.c_ly[u] + bs.c_ly[v], lz = bs.c_lz[u] + bs.c_lz[v];
                const int c = (lx & 1) | ((ly & 1) << 1);
                slab.pairW[p][c] += (double)((lx / 2 + 1) * (ly / 2 + 1) * (lz + 1));
                slab.pairNc[p][c] += 1.0;
            }
    }
    // prefix sums over the first shell A of the ket pairs (the pair list is A-major): npp x W per class, and npp x n per class and Lc + Ld
    slab.cumW.assign(sto.nsh + 1, std::array<double, 4>{0, 0, 0, 0});
    slab.cumNL.resize(sto.nsh + 1);
    for (auto &x : slab.cumNL) x.fill(0.0);
    for (int p = 0; p < sto.npairs; ++p) {
        const int A = bs.pairs[p].A, lcd = std::min(10, bs.pairs[p].La + bs.pairs[p].Lb);
        for (int c = 0; c < 4; ++c) {
            slab.cumW[A + 1][c] += (double)bs.pairs[p].npp * slab.pairW[p][c];
            slab.cumNL[A + 1][4 * lcd + c] += (double)bs.pairs[p].npp * slab.pairNc[p][c];
        }
    }
    for (int a = 0; a < sto.nsh; ++a) {
        for (int c = 0; c < 4; ++c) slab.cumW[a + 1][c] += slab.cumW[a][c];
        for (int x = 0; x < 44; ++x) slab.cumNL[a + 1][x] += slab.cumNL[a][x];
    }
}

int EriBuild::plan_ket_lists()
{
    int rc;
    // class-sorted ket lists on the device (one contiguous range per class)
    sto.ncls = (int)ctx->class_pairs.size();
    kets.ket_off.assign(sto.ncls + 1, 0); kets.cls_maxnpp.assign(sto.ncls, 1);
    for (int c = 0; c < sto.ncls; ++c) {
        kets.ket_sorted.insert(kets.ket_sorted.end(), ctx->class_pairs[c].begin(), ctx->class_pairs[c].end());
        kets.ket_off[c + 1] = (int)kets.ket_sorted.size();
        for (int p : ctx->class_pairs[c]) kets.cls_maxnpp[c] = std::max(kets.cls_maxnpp[c], bs.pairs[p].npp);
    }
    if ((rc = mem.up(kets.ket_sorted, &kets.d_kets))) return rc;
    {
        // generic (single-launch) mode: heaviest ket pairs first -- workgroups are dispatched in index order, and a deeply contracted
        // (pp|pp) quartet of Ar2/cc-pVQZ runs for 12 ms: it has to start early, not at the tail of the launch
        // the launches are made per (bra group, ket group) of shell pairs -- groups by La + Lb -- so that the LDS carve-out of each
        // launch fits its own angular momenta (the (gg|gg) tables need 100 KB, the (ss|ss) ones nothing)
        std::vector<int> all(sto.npairs);
        std::iota(all.begin(), all.end(), 0);
        std::stable_sort(all.begin(), all.end(), [&](int x, int y) {
            const int gx = pair_group(x), gy = pair_group(y);
            return gx != gy ? gx < gy : pair_cost(x) > pair_cost(y);
        });
        for (int p : all) ++kets.kets_goff[pair_group(p) + 1];
        for (int g = 0; g < NGRP; ++g) kets.kets_goff[g + 1] += kets.kets_goff[g];
        if ((rc = mem.up(all, &kets.d_kets_all))) return rc;
        kets.kets_all_host = all;
    }
    return TF_OK;
}

// Families of ket pairs (general contractions, eri_cfact_kernel<.., MM>): shells with identical primitives -- same centre, L, exponents,
// components -- get the same primitive-set id; the contracted pairs of a group with the same (id, id) differ only in their primitive-pair
// weights and in the AOs they write.  Per contracted group: heads (first member, the group's cost order kept), members of each head.
int EriBuild::plan_ket_families()
{
    int rc;
    // (on when the build has the work to fill the chip with fewer, longer workgroups: Ar2/cc-pVQZ -- 5.0e7 primitive shell quartets -- gains
    // 20 %, N2/cc-pVTZ -- 1.2e6 -- loses 20 %; TF_ERI_FAMILIES=0 / 1 forces)
    const double prim_quartets_est = 0.5 * (double)slab.cum_pp[sto.nsh] * (double)slab.cum_pp[sto.nsh];
    kets.fam_off = knobs.families >= 0 ? knobs.families == 0 : prim_quartets_est < 8.0e6;
    std::vector<int> fam_heads, fam_ptr{0}, fam_mem;
    kets.bra_fam_on = !kets.fam_off && knobs.bra_fam;
    kets.psid.assign(bs.shells.size(), -1);
    {
        int nid = 0;
        for (size_t a = 0; a < bs.shells.size(); ++a) {
            if (kets.psid[a] >= 0) continue;
            kets.psid[a] = nid;
            const tf::Shell &sa = bs.shells[a];
            for (size_t b = a + 1; b < bs.shells.size(); ++b) {
                const tf::Shell &sb = bs.shells[b];
                if (kets.psid[b] >= 0 || sb.z != sa.z || sb.L != sa.L || sb.nprim != sa.nprim || sb.ncomp != sa.ncomp || sb.full != sa.full) continue;
                bool same = true;
                for (int q = 0; q < sa.nprim && same; ++q) same = bs.s_exp[sa.prim_off + q] == bs.s_exp[sb.prim_off + q];
                for (int q = 0; q < sa.ncomp && same; ++q)
                    same = bs.c_lx[sa.comp_off + q] == bs.c_lx[sb.comp_off + q] && bs.c_ly[sa.comp_off + q] == bs.c_ly[sb.comp_off + q] &&
                           bs.c_lz[sa.comp_off + q] == bs.c_lz[sb.comp_off + q] && bs.c_scale[sa.comp_off + q] == bs.c_scale[sb.comp_off + q];
                if (same) kets.psid[b] = nid;
            }
            ++nid;
        }
        for (int g = 0; g < NGRP; ++g) {
            kets.fam_goff[g] = (int)fam_heads.size();
            if (!(g & 1) || kets.fam_off) continue;                     // contracted groups only
            std::map<std::pair<int, int>, std::vector<int>> open_fam;   // key -> index of the family still taking members (in fam_ptr order)
            std::vector<std::vector<int>> fams;
            for (int k = kets.kets_goff[g]; k < kets.kets_goff[g + 1]; ++k) {
                const int p = kets.kets_all_host[k];
                const auto key = std::make_pair(kets.psid[bs.pairs[p].A], kets.psid[bs.pairs[p].B]);
                auto it = open_fam.find(key);
                if (it == open_fam.end() || (int)fams[it->second.back()].size() >= FAM_MM) {
                    fams.emplace_back();
                    open_fam[key].push_back((int)fams.size() - 1);
                    it = open_fam.find(key);
                }
                fams[it->second.back()].push_back(p);
            }
            for (const auto &f : fams) {
                fam_heads.push_back(f[0]);
                fam_mem.insert(fam_mem.end(), f.begin(), f.end());
                fam_ptr.push_back((int)fam_mem.size());
                if (f.size() > 1) kets.fam_any = true;
            }
        }
        kets.fam_goff[NGRP] = (int)fam_heads.size();
        if (kets.fam_any) {
            if ((rc = mem.up(fam_heads, &kets.d_fam_heads)) || (rc = mem.up(fam_ptr, &kets.d_fam_ptr)) ||
                (rc = mem.up(fam_mem, &kets.d_fam_mem)))
                return rc;
        }
    }
    return TF_OK;
}

// streams so that the many small class launches of a slab overlap
int EriBuild::setup_streams()
{
    run.NSTREAM = knobs.nstream;
    HIPCHK(ctx, (hipError_t)ctx->bstr.create());                 // (all of them or none; made once per context)
    run.streams = ctx->bstr.streams;
    run.sev = ctx->bstr.sev;
    return TF_OK;
}

// the class-wide part of a team kernel's class record (tf_eri_team.hip.h) for (bra pair class, ket pair class)
TClass EriBuild::tclass_common(int bcls, int kcls, int &maxblk, int &maxK, int &nnzc) const
{
    const DPair &hb = ctx->host_pairs[ctx->class_pairs[bcls][0]], &hk = ctx->host_pairs[ctx->class_pairs[kcls][0]];
    const KClassTab &kt = tt.kct[kcls];
    TClass t{};
    t.La = hb.La; t.Lb = hb.Lb; t.Lc = hk.La; t.Ld = hk.Lb;
    t.nTab = (t.La + 1) * (t.Lb + 1); t.nTcd = (t.Lc + 1) * (t.Ld + 1); t.nT = t.nTab * t.nTcd;
    t.inv_nTcd = 1.0f / (float)t.nTcd;
    t.nab = hb.nca * hb.ncb; t.ncd = hk.nca * hk.ncb;
    maxblk = 1; maxK = 1; nnzc = 0;
    for (int i = 0; i < 5; ++i) { t.pA[i] = hb.pcls[i]; t.pK[i] = hk.pcls[i]; t.pS[i] = kt.pS[i]; }
    for (int i = 0; i < 4; ++i) {
        maxK = std::max(maxK, t.pK[i + 1] - t.pK[i]);
        maxblk = std::max(maxblk, (t.pA[i + 1] - t.pA[i]) * (t.pK[i + 1] - t.pK[i]));
        nnzc += (t.pA[i + 1] - t.pA[i]) * (t.pK[i + 1] - t.pK[i]);
    }
    t.nkap = kt.nkap; t.nnzT = kt.nnzT; t.tabA = hb.tab_off; t.tabK = hk.tab_off; t.ktp_off = kt.tp_off; t.kte_off = kt.te_off;
    t.nEab = hb.nE; t.nEcd = hk.nE; t.RLS = H.RLS; t.nacc = nnzc;
    t.nout = 0;
    for (int i = 0; i < 4; ++i) {
        t.invK[i] = 1.0f / (float)std::max(1, t.pK[i + 1] - t.pK[i]);
        t.invS[i] = 1.0f / (float)std::max(1, t.pS[i + 1] - t.pS[i]);
        t.nout += (t.pA[i + 1] - t.pA[i]) * (t.pS[i + 1] - t.pS[i]);
    }
    return t;
}

// bra_Amax: largest first shell among the bra pairs of the run -- in the packed layout only kets with first shell <= it are needed
// (the class ket lists ascend in the first shell, so that is a prefix: workgroups beyond it are not even launched)
void EriBuild::launch_class(int bcls, int kcls, int max_npp_bra, unsigned n_bra, const int *d_bra, const long long *d_braoff, int bra_Amax)
{
    const tf::Pair &pb = bs.pairs[ctx->class_pairs[bcls][0]], &pk = bs.pairs[ctx->class_pairs[kcls][0]];
    const tf::Shell &sa = bs.shells[pb.A], &sb = bs.shells[pb.B], &sc = bs.shells[pk.A], &sd = bs.shells[pk.B];
    QClass q{};
    q.La = pb.La; q.Lb = pb.Lb; q.Lc = pk.La; q.Ld = pk.Lb;
    q.L = q.La + q.Lb + q.Lc + q.Ld;
    q.tsize = (q.L + 1) * (q.L + 2) / 2;
    q.nca = sa.ncomp; q.ncb = sb.ncomp; q.ncc = sc.ncomp; q.ncd = sd.ncomp;
    q.ncomp = q.nca * q.ncb * q.ncc * q.ncd;
    q.npp_ab = max_npp_bra; q.npp_cd = kets.cls_maxnpp[kcls]; q.npq = q.npp_ab * q.npp_cd;      // class maxima (LDS sizing)
    q.nEab = pb.nE; q.nEcd = pk.nE;
    q.n_ket = kets.ket_off[kcls + 1] - kets.ket_off[kcls];
    if (sto.packed) {
        const std::vector<int> &kl = ctx->class_pairs[kcls];
        q.n_ket = (int)(std::upper_bound(kl.begin(), kl.end(), bra_Amax, [&](int a, int p) { return a < bs.pairs[p].A; }) - kl.begin());
        if (q.n_ket == 0) return;
    }
    q.fused = 1; q.spherical = spherical ? 1 : 0;
    q.nsc = spherical ? sc.nsph : sc.ncomp; q.nsd = spherical ? sd.nsph : sd.ncomp;
    q.Nout = sto.N; q.ld = sto.ld;
    q.tri = sto.packed ? 1 : 0;
    double *d_out_slab = slab.d_T2;                               // fused kernels write the half-transformed slab directly
    const int *d_ket = kets.d_kets + kets.ket_off[kcls];
    hipStream_t st = run.streams[run.launch_count++ % run.NSTREAM];
    ClassTimer class_timer(EriKnobs::class_times(), q, n_bra);
    if (lt.use_team_pc && q.npq == 1 && q.La + q.Lb <= TF_TEAM_LMAX && q.Lc + q.Ld <= TF_TEAM_LMAX) {
        // one shell quartet per team of lanes, tables private to the team (tf_eri_team.hip.h)
        int maxblk = 1, maxK = 1, nnzc = 0;
        TClass t = tclass_common(bcls, kcls, maxblk, maxK, nnzc);
        t.n_ket = q.n_ket;
        const int LAB = q.La + q.Lb, LCD = q.Lc + q.Ld;
        const tfe::TeamSizes S = tfe::carve_team(t, tt.flat_off.empty() ? -1 : tt.flat_off[(size_t)bcls * sto.ncls + kcls], maxblk, maxK, nnzc);
        const bool avail[3] = {eri_team_available(LAB, LCD, 16), eri_team_available(LAB, LCD, 64), eri_team_available(LAB, LCD, 256)};
        const int team = tfe::choose_team(avail, S.bytes, t.nT, nnzc, (size_t)EriKnobs::team_lds_kb() * 1024, EriKnobs::team16_nnz(), EriKnobs::team_size());
        if (team) {
            tfe::team_apply(t, S, team);
            const unsigned gx = tfe::team_grid_x(q.n_ket, team, n_bra, EriKnobs::team_kpw_div(), EriKnobs::team_kpw_max());
            TeamLaunch a{LAB, LCD, team, dim3(gx, n_bra), S.bytes[tfe::team_slot(team)], st, &ctx->db, &t,
                         tt.d_brarec + (d_bra - tt.d_bra_base), tt.d_ketrec + kets.ket_off[kcls], tt.d_kcnt + (size_t)kcls * sto.nsh, d_out_slab};
            const hipError_t e = eri_team_launch(a);
            if (e != hipSuccess) { lt.team_error = e; }
            count(team == 16 ? TF_ERI_STAT_TEAM16 : (team == 64 ? TF_ERI_STAT_TEAM64 : TF_ERI_STAT_TEAM256));
            if (t.flat) ++run.stats[TF_ERI_STAT_TEAM_FLAT];
            return;
        }
    }
    if (q.npq == 1 && q.ncomp <= 128) {
        tfe::carve_multi(q);
        const dim3 grid((q.n_ket + q.G - 1) / q.G, n_bra);
        count(TF_ERI_STAT_MULTI);
        hipLaunchKernelGGL(eri_multi_kernel, grid, dim3(TF_ERI_THREADS), tfe::lds_bytes(q.lds_doubles), st, ctx->db, q, d_bra, d_braoff,
                           d_ket, sto.Nc, d_out_slab);
    } else if (q.npq == 1 && (q.La + 1) * (q.Lb + 1) * (q.Lc + 1) * (q.Ld + 1) * 2 * (q.L / 2 + 1) <= 7000 && !knobs.nofact) {
        const LRec &lr = lt.lrecs_host[((q.La * 6 + q.Lb) * 6 + q.Lc) * 6 + q.Ld];
        tfe::carve_fact(q, lr.tupG_off, lr.tupXZ_off);
        count(TF_ERI_STAT_FACT);
        hipLaunchKernelGGL(eri_fact_kernel, dim3(q.n_ket, n_bra), dim3(EriKnobs::fact_threads()), tfe::lds_bytes(q.lds_doubles), st, ctx->db, q, d_bra,
                           d_braoff, d_ket, sto.Nc, d_out_slab);
    } else {
        const bool stage = tfe::carve_class(q);
        const dim3 grid(q.n_ket, n_bra);
        count(stage ? TF_ERI_STAT_CLASS_STAGED : TF_ERI_STAT_CLASS_UNSTAGED);
        if (stage)
            hipLaunchKernelGGL((eri_class_kernel<true, false>), grid, dim3(TF_ERI_THREADS), tfe::lds_bytes(q.lds_doubles), st, ctx->db, q,
                               d_bra, d_braoff, d_ket, sto.Nc, d_out_slab);
        else
            hipLaunchKernelGGL((eri_class_kernel<false, false>), grid, dim3(TF_ERI_THREADS), tfe::lds_bytes(q.lds_doubles), st, ctx->db, q,
                               d_bra, d_braoff, d_ket, sto.Nc, d_out_slab);
    }
}

// Small problems: per slab one launch per (bra group, ket group), each mixing the classes of its groups (LDS carved by the
// capacities the groups need).  bra_host: the slab's bra pairs (sorted by group).
void EriBuild::launch_generic_old(unsigned n_bra, const int *d_bra, const long long *d_braoff, unsigned n_ket, const int *d_ket, hipStream_t st)
{
    QClass q{};
    tfe::carve_component_lane(q);
    q.n_ket = (int)n_ket; q.fused = 0;
    q.tri = sto.packed ? 1 : 0;
    count(TF_ERI_STAT_COMPONENT_LANE);
    hipLaunchKernelGGL((eri_class_kernel<true, true>), dim3(n_ket, n_bra), dim3(TF_ERI_THREADS), tfe::lds_bytes(q.lds_doubles), st,
                       ctx->db, q, d_bra, d_braoff, d_ket, sto.Nc, slab.d_C);
}

tfe::GroupStat EriBuild::group_stat(const int *pairs_host, size_t n) const
{
    tfe::GroupStat g;
    for (size_t k = 0; k < n; ++k) {
        const tf::Pair &pr = bs.pairs[pairs_host[k]];
        tfe::group_stat(g, pr.La, pr.Lb, pr.npp, pr.nE, bs.shells[pr.A].ncomp * bs.shells[pr.B].ncomp);
    }
    return g;
}

// LDS carve-out of the launch (bra group gb, ket group gk), from the largest angular momenta / contraction depths of the groups
void EriBuild::make_caps()
{
    tfe::GroupStat gs[NGRP];
    for (int g = 0; g < NGRP; ++g) gs[g] = group_stat(kets.kets_all_host.data() + kets.kets_goff[g], (size_t)(kets.kets_goff[g + 1] - kets.kets_goff[g]));
    for (int gb = 0; gb < NGRP; ++gb)
        for (int gk = 0; gk < NGRP; ++gk) {
            const tfe::CFPlan P = tfe::carve_cfact(gs[gb], gs[gk], gb & 1, gk & 1, EriKnobs::cfact(), kets.fam_off ? 0 : FAM_MM, sto.packed,
                                                   lt.use_teamc ? TF_TEAM_LMAX : -1, lt.teamc_pqmax);
            lt.gcaps[gb][gk] = P.caps; lt.gcaps_fit[gb][gk] = P.fit; lt.gcaps_gtab[gb][gk] = P.gtab;
            lt.gcaps[gb][gk].dbg_npq_lo = knobs.dbg_npq_lo; lt.gcaps[gb][gk].dbg_npq_hi = knobs.dbg_npq_hi;
        }
}

// per (La, Lb | Lc, Ld): table sizes, index words of the table entries, batch capacity under the caps of its launch
int EriBuild::make_lrecs(bool with_caps)
{
    std::vector<LRec> recs(6 * 6 * 6 * 6, LRec{});
    std::vector<unsigned short> tup;
    std::vector<char> seen_pair(36, 0);
    for (const tf::Pair &pr : bs.pairs) seen_pair[pr.La * 6 + pr.Lb] = 1;
    for (int ab = 0; ab < 36; ++ab)
        for (int cd = 0; cd < 36; ++cd) {
            if (!seen_pair[ab] || !seen_pair[cd]) continue;
            const int La = ab / 6, Lb = ab % 6, Lc = cd / 6, Ld = cd % 6;
            const int gb = tfe::lp_group(La + Lb), gk = tfe::lp_group(Lc + Ld);
            LRec r = tfe::lrec_sizes(La, Lb, Lc, Ld);
            // batch capacity: the smallest over the launches (contracted bra and / or ket group) this tuple can occur in
            for (int fb = 0; fb < 2 && with_caps; ++fb)
                for (int fk = 0; fk < 2; ++fk)
                    if (fb + fk) tfe::lrec_limit(r, lt.gcaps[2 * gb + fb][2 * gk + fk]);
            r.tupG_off = (int)tup.size();
            r.tupXZ_off = r.tupG_off + r.gsz;
            tup.resize(tup.size() + (size_t)r.gsz + (size_t)r.xz);
            tfe::lrec_words(r, La, Lb, Lc, Ld, tup.data() + r.tupG_off);
            recs[ab * 36 + cd] = r;
        }
    int rc2;
    if ((rc2 = upload(ctx, recs, CB_LREC)) || (rc2 = upload(ctx, tup, CB_TUP))) return rc2;
    ctx->db.lrec = ctx->blk.at<LRec>(CB_LREC); ctx->db.tup = ctx->blk.at<unsigned short>(CB_TUP);
    lt.lrecs_host = recs;
    return TF_OK;
}

// families of the bra pairs [b0, b1) of the slab's list, at most `most` members each: built and uploaded once per (slab, bra group)
const EriBuild::BraFam *EriBuild::bra_families(BraFams &bra_fams, const std::vector<int> &bra_host, size_t b0, size_t b1, int most)
{
    auto bf = bra_fams.find(std::make_pair(b0, most));
    if (bf != bra_fams.end()) return &bf->second;
    BraFam nf;
    std::vector<int> bptr{0}, bmem;
    std::map<std::pair<int, int>, int> open_fam;
    std::vector<std::vector<int>> fams;
    for (size_t y = b0; y < b1; ++y) {
        const tf::Pair &pr = bs.pairs[bra_host[y]];
        const auto key = std::make_pair(kets.psid[pr.A], kets.psid[pr.B]);
        auto it = open_fam.find(key);
        if (it == open_fam.end() || (int)fams[it->second].size() >= most) {
            fams.emplace_back();
            open_fam[key] = (int)fams.size() - 1;
            it = open_fam.find(key);
        }
        fams[it->second].push_back((int)y);
    }
    for (const auto &f : fams) { bmem.insert(bmem.end(), f.begin(), f.end()); bptr.push_back((int)bmem.size()); }
    if (mem.up(bptr, &nf.d_ptr) || mem.up(bmem, &nf.d_mem)) return nullptr;
    nf.n = (unsigned)(bptr.size() - 1);
    return &bra_fams.emplace(std::make_pair(b0, most), nf).first->second;
}

// One launch per (bra group, ket group) with work.  A process has few hardware queues (4 by default) and the launches of one
// queue run one after the other, each as long as its slowest workgroup: the launches are spread over NQ streams by estimated
// cost (heaviest first, always onto the least loaded stream) instead of round-robin over all of them.
int EriBuild::launch_generic(const std::vector<int> &bra_host, const int *d_bra, const long long *d_braoff)
{
    const bool old_generic = EriKnobs::generic_old();
    struct Launch { size_t b0, b1; int gb, gk; double cost; };
    std::vector<Launch> launches;
    double ket_cost[NGRP];
    for (int g = 0; g < NGRP; ++g) {
        ket_cost[g] = 0.0;
        for (int k = kets.kets_goff[g]; k < kets.kets_goff[g + 1]; ++k) ket_cost[g] += (double)pair_cost(kets.kets_all_host[k]);
    }
    for (size_t b0 = 0; b0 < bra_host.size();) {
        const int gb = pair_group(bra_host[b0]);
        size_t b1 = b0;
        double bc = 0.0;
        while (b1 < bra_host.size() && pair_group(bra_host[b1]) == gb) { bc += (double)pair_cost(bra_host[b1]); ++b1; }
        for (int gk = 0; gk < NGRP; ++gk)
            if (kets.kets_goff[gk + 1] > kets.kets_goff[gk]) launches.push_back(Launch{b0, b1, gb, gk, bc * ket_cost[gk]});
        b0 = b1;
    }
    std::stable_sort(launches.begin(), launches.end(), [](const Launch &x, const Launch &y) { return x.cost > y.cost; });
    const int NQ = std::min(run.NSTREAM, knobs.nq);
    std::vector<double> load(NQ, 0.0);
    BraFams bra_fams;
    for (const Launch &l : launches) {
        const int qi = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        load[qi] += l.cost;
        hipStream_t st = run.streams[qi];
        const int gb = l.gb, gk = l.gk, nk = kets.kets_goff[gk + 1] - kets.kets_goff[gk];
        const size_t b0 = l.b0, b1 = l.b1;
        const CFCaps &c = lt.gcaps[gb][gk];
        const size_t bytes = (size_t)c.lds_doubles * sizeof(double);
        if (old_generic || !lt.gcaps_fit[gb][gk]) {             // the component-per-lane kernel
            launch_generic_old((unsigned)(b1 - b0), d_bra + b0, d_braoff + b0, (unsigned)nk, kets.d_kets_all + kets.kets_goff[gk], st);
            continue;
        }
        if (bytes > 64 * 1024 && !ctx->cfact_lds_set) {
            HIPCHK(ctx, hipFuncSetAttribute((const void *)eri_cfact_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tfe::ERI_LDS_MAX_BYTES));
            HIPCHK(ctx, hipFuncSetAttribute((const void *)eri_cfact_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tfe::ERI_LDS_MAX_BYTES));
            HIPCHK(ctx, hipFuncSetAttribute((const void *)eri_cfact_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tfe::ERI_LDS_MAX_BYTES));
            ctx->cfact_lds_set = 160 * 1024;
        }
        if (lt.gcaps_gtab[gb][gk]) {
            const size_t need = (size_t)nk * (b1 - b0) * (size_t)c.gtab_doubles * sizeof(double);
            if (need > ctx->blk.cap[CB_GTAB]) {
                HIPCHK(ctx, hipDeviceSynchronize());           // (earlier launches of this build may still use the old block)
                HIPCHK(ctx, (hipError_t)ctx->blk.ensure(CB_GTAB, need));
            }
            // launches that share the block must not overlap: they all go to one stream
            count(TF_ERI_STAT_CFACT_GTAB);
            hipLaunchKernelGGL((eri_cfact_kernel<true, true>), dim3((unsigned)nk, (unsigned)(b1 - b0)), dim3(TF_ERI_THREADS), bytes, run.streams[0], ctx->db, c,
                               d_bra + b0, d_braoff + b0, kets.d_kets_all + kets.kets_goff[gk], sto.Nc, slab.d_C, ctx->d_gtab());
            load[qi] -= l.cost; load[0] += l.cost;
        } else if (((gb | gk) & 1) == 0) {                   // both groups uncontracted: one primitive quartet per shell quartet
            count(TF_ERI_STAT_CFACT_UNCONTRACTED);
            hipLaunchKernelGGL(eri_cfact_kernel<true>, dim3((unsigned)nk, (unsigned)(b1 - b0)), dim3(TF_ERI_THREADS), bytes, st, ctx->db, c,
                               d_bra + b0, d_braoff + b0, kets.d_kets_all + kets.kets_goff[gk], sto.Nc, slab.d_C);
        } else if ((gb & 1) && !(gk & 1) && kets.bra_fam_on) {       // contracted bras against uncontracted kets: (family of bra pairs, ket pair).
            // Off by default (TF_ERI_BRA_FAMILIES=1): the packed layout evaluates the kets whose first shell does not exceed the bra's,
            // and the contracted shells come first on each atom -- the contracted pairs sit on the ket side; measured on Ar2/cc-pVQZ these
            // bra families cost 5 % (fewer, longer workgroups) where the ket families gain 24 %.
            const BraFam *bf = bra_families(bra_fams, bra_host, b0, b1, FAM_MM);
            if (!bf) return TF_ENOMEM;
            static bool bfam_attr_set = false;
            if (bytes > 64 * 1024 && !bfam_attr_set) {
                HIPCHK(ctx, hipFuncSetAttribute((const void *)eri_cfact_kernel<false, false, FAM_MM, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tfe::ERI_LDS_MAX_BYTES));
                bfam_attr_set = true;
            }
            count(TF_ERI_STAT_CFACT_BRA_FAMILIES);
            hipLaunchKernelGGL((eri_cfact_kernel<false, false, FAM_MM, 1>), dim3((unsigned)nk, bf->n), dim3(TF_ERI_THREADS), bytes, st,
                               ctx->db, c, d_bra, d_braoff, kets.d_kets_all + kets.kets_goff[gk], sto.Nc, slab.d_C, (double *)nullptr, (const int *)nullptr,
                               (const int *)nullptr, bf->d_ptr, bf->d_mem);
        }
        else if ((gb & 1) && (gk & 1) && kets.fam_any && !knobs.cc_fam_off) {
            // contracted against contracted: families on both sides -- up to 3 bra pairs x up to 9 ket pairs per workgroup (27 accumulators
            // per component: the deepest quartets, (s13 s13|s13 s13) and friends, spend their time in the tables of 28 561 primitive quartets)
            const BraFam *bf = bra_families(bra_fams, bra_host, b0, b1, FAM_MA_CC);
            if (!bf) return TF_ENOMEM;
            static bool ccfam_attr_set = false;
            if (bytes > 64 * 1024 && !ccfam_attr_set) {
                HIPCHK(ctx, hipFuncSetAttribute((const void *)eri_cfact_kernel<false, false, FAM_MA_CC, FAM_MM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tfe::ERI_LDS_MAX_BYTES));
                ccfam_attr_set = true;
            }
            count(TF_ERI_STAT_CFACT_BOTH_FAMILIES);
            hipLaunchKernelGGL((eri_cfact_kernel<false, false, FAM_MA_CC, FAM_MM>), dim3((unsigned)(kets.fam_goff[gk + 1] - kets.fam_goff[gk]), bf->n),
                               dim3(TF_ERI_THREADS), bytes, st, ctx->db, c, d_bra, d_braoff, kets.d_fam_heads + kets.fam_goff[gk], sto.Nc, slab.d_C, (double *)nullptr,
                               kets.d_fam_ptr + kets.fam_goff[gk], kets.d_fam_mem, bf->d_ptr, bf->d_mem);
        }
        else if ((gk & 1) && kets.fam_any) {                       // contracted kets: one workgroup per (bra pair, family of ket pairs)
            static bool fam_attr_set = false;                 // (per process and device: the attribute belongs to the function)
            if (bytes > 64 * 1024 && !fam_attr_set) {
                HIPCHK(ctx, hipFuncSetAttribute((const void *)eri_cfact_kernel<false, false, 1, FAM_MM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tfe::ERI_LDS_MAX_BYTES));
                fam_attr_set = true;
            }
            count(TF_ERI_STAT_CFACT_KET_FAMILIES);
            hipLaunchKernelGGL((eri_cfact_kernel<false, false, 1, FAM_MM>), dim3((unsigned)(kets.fam_goff[gk + 1] - kets.fam_goff[gk]), (unsigned)(b1 - b0)),
                               dim3(TF_ERI_THREADS), bytes, st, ctx->db, c, d_bra + b0, d_braoff + b0, kets.d_fam_heads + kets.fam_goff[gk], sto.Nc, slab.d_C,
                               (double *)nullptr, kets.d_fam_ptr + kets.fam_goff[gk], kets.d_fam_mem);
        } else {
            count(TF_ERI_STAT_CFACT_CONTRACTED);
            hipLaunchKernelGGL(eri_cfact_kernel<false>, dim3((unsigned)nk, (unsigned)(b1 - b0)), dim3(TF_ERI_THREADS), bytes, st, ctx->db, c,
                               d_bra + b0, d_braoff + b0, kets.d_kets_all + kets.kets_goff[gk], sto.Nc, slab.d_C);
        }
        ++run.launch_count;
    }
    return TF_OK;
}

// ---- team kernels (tf_eri_team.hip.h): the uncontracted classes of the per-class mode, packed layout.  Per pair class the ket
// pair transform (Cartesian component pairs -> output pairs inside each x/y parity class, normalisation ratios folded in), per
// shell pair the slab offsets of its output pairs.
int EriBuild::plan_team_tables()
{
    int rc;
    if (!lt.use_team) return TF_OK;
    int *d_kq_ptr = nullptr, *d_kq_off = nullptr, *d_kt_ptr = nullptr, *d_kt_k = nullptr, *d_tflat = nullptr;
    double *d_kt_c = nullptr;
    std::vector<int> kt_ptr, kt_k, kq_ptr(sto.npairs, 0), kq_off;
    std::vector<double> kt_c, blkC, blkD;
    std::vector<std::vector<int>> kap_list(sto.ncls);               // output pairs (sc << 8 | sd) of a pair class, sorted by parity class
    auto rows_of = [&](const tf::Shell &sh, std::vector<double> &U) {   // transformation rows of a shell (identity: Cartesian output)
        if (spherical) { tf::sph_block(sh.L, U); return; }
        U.assign((size_t)sh.ncomp * sh.ncomp, 0.0);
        for (int i = 0; i < sh.ncomp; ++i) U[(size_t)i * sh.ncomp + i] = 1.0;
    };
    auto cls_of = [&](const tf::Shell &sh, const std::vector<double> &U, int r) {   // parity class of an output function: its first component's
        int cc = 0;
        while (cc + 1 < sh.ncomp && U[(size_t)r * sh.ncomp + cc] == 0.0) ++cc;
        const int a = sh.comp_off + cc;
        return (bs.c_lx[a] & 1) | ((bs.c_ly[a] & 1) << 1);
    };
    for (int c = 0; c < sto.ncls; ++c) {
        const DPair &pr = ctx->host_pairs[ctx->class_pairs[c][0]];
        const tf::Shell &sC = bs.shells[pr.A], &sD = bs.shells[pr.B];
        const int nsc = out_dim(sC), nsd = out_dim(sD), ncc = sC.ncomp, ncd = sD.ncomp;
        rows_of(sC, blkC); rows_of(sD, blkD);
        std::vector<int> loc((size_t)ncc * ncd, 0);              // position of a component pair inside its parity class (inverse of ct_ord)
        for (int cl = 0; cl < 4; ++cl)
            for (int s2 = pr.pcls[cl]; s2 < pr.pcls[cl + 1]; ++s2) loc[ctx->h_ct_ord[pr.tab_off + s2]] = s2 - pr.pcls[cl];
        KClassTab &kt = tt.kct[c];
        kt.tp_off = (int)kt_ptr.size(); kt.te_off = (int)kt_k.size();
        for (int cl = 0; cl < 4; ++cl) {
            kt.pS[cl] = (int)kap_list[c].size();
            for (int sc = 0; sc < nsc; ++sc)
                for (int sd = 0; sd < nsd; ++sd) {
                    if ((cls_of(sC, blkC, sc) ^ cls_of(sD, blkD, sd)) != cl) continue;
                    kap_list[c].push_back((sc << 8) | sd);
                    kt_ptr.push_back((int)kt_k.size() - kt.te_off);
                    for (int cc = 0; cc < ncc; ++cc) {
                        const double uc = blkC[(size_t)sc * ncc + cc];
                        if (uc == 0.0) continue;
                        for (int cd2 = 0; cd2 < ncd; ++cd2) {
                            const double ud = blkD[(size_t)sd * ncd + cd2];
                            if (ud == 0.0) continue;
                            const int f = cc * ncd + cd2;
                            kt_k.push_back(loc[f]);
                            kt_c.push_back(uc * ud * ctx->h_ct_sc[pr.tab_off + f]);
                        }
                    }
                }
        }
        kt.pS[4] = kt.nkap = (int)kap_list[c].size();
        kt_ptr.push_back((int)kt_k.size() - kt.te_off);
        kt.nnzT = (int)kt_k.size() - kt.te_off;
    }
    for (int p = 0; p < sto.npairs; ++p) {
        const DPair &pr = ctx->host_pairs[p];
        kq_ptr[p] = (int)kq_off.size();
        for (int word : kap_list[ctx->pair_class[p]]) {
            const int k = pr.outoff_a + (word >> 8), l = pr.outoff_b + (word & 255);
            if (l > k) { kq_off.push_back(-1); continue; }
            const int cb = H.cls[k] ^ H.cls[l];
            kq_off.push_back(H.fullsec[cb][H.cls[k]] + H.kinfo[(size_t)cb * sto.N + H.sigma[k]].offA + H.loc[l]);
        }
    }
    if ((rc = mem.up(kq_ptr, &d_kq_ptr)) || (rc = mem.up(kq_off, &d_kq_off)) || (rc = mem.up(kt_ptr, &d_kt_ptr)) ||
        (rc = mem.up(kt_k, &d_kt_k)) || (rc = mem.up(kt_c, &d_kt_c)))
        return rc;
    ctx->db.kq_ptr = d_kq_ptr; ctx->db.kq_off = d_kq_off; ctx->db.kt_ptr = d_kt_ptr; ctx->db.kt_k = d_kt_k; ctx->db.kt_c = d_kt_c;
    // flat records of the class-sorted ket list (uncontracted pairs) and, per class and shell A, the kets with first shell <= A
    std::vector<KetRec> krec(kets.ket_sorted.size());
    for (size_t k = 0; k < kets.ket_sorted.size(); ++k) {
        const tf::Pair &pr = bs.pairs[kets.ket_sorted[k]];
        const double qq = bs.pp_p[pr.pp_off];
        krec[k] = KetRec{qq, bs.pp_Pz[pr.pp_off], bs.pp_K[pr.pp_off] / qq, (unsigned)pr.e_off, kq_ptr[kets.ket_sorted[k]]};
    }
    std::vector<int> kcnt((size_t)sto.ncls * sto.nsh, 0);
    for (int c = 0; c < sto.ncls; ++c) {
        for (int p2 : ctx->class_pairs[c]) ++kcnt[(size_t)c * sto.nsh + bs.pairs[p2].A];
        for (int a = 1; a < sto.nsh; ++a) kcnt[(size_t)c * sto.nsh + a] += kcnt[(size_t)c * sto.nsh + a - 1];
    }
    if ((rc = mem.up(krec, &tt.d_ketrec)) || (rc = mem.up(kcnt, &tt.d_kcnt))) return rc;
    if (lt.use_team_pc) {
        // flat lists of the parity-allowed components and of the outputs of every (bra class, ket class) of uncontracted pairs
        std::vector<int> tflat;
        tt.flat_off.assign((size_t)sto.ncls * sto.ncls, -1);
        for (int bc = 0; bc < sto.ncls; ++bc)
            for (int kc = 0; kc < sto.ncls; ++kc) {
                const DPair &hb = ctx->host_pairs[ctx->class_pairs[bc][0]], &hk = ctx->host_pairs[ctx->class_pairs[kc][0]];
                if (hb.npp != 1 || hk.npp != 1 || hb.La + hb.Lb > TF_TEAM_LMAX || hk.La + hk.Lb > TF_TEAM_LMAX) continue;
                int mb, mk, nz;
                const TClass t = tclass_common(bc, kc, mb, mk, nz);
                if (nz > 2048) continue;                          // (chunked classes keep the loop per parity class)
                tt.flat_off[(size_t)bc * sto.ncls + kc] = (int)tflat.size();
                for (int c = 0; c < 4; ++c)
                    for (int il = 0; il < t.pA[c + 1] - t.pA[c]; ++il)
                        for (int kl = 0; kl < t.pK[c + 1] - t.pK[c]; ++kl) tflat.push_back((t.pA[c] + il) | ((t.pK[c] + kl) << 16));
                if (tflat.size() & 1) tflat.push_back(0);
                int vbase = 0;
                for (int c = 0; c < 4; ++c) {
                    const int nA = t.pA[c + 1] - t.pA[c], nK = t.pK[c + 1] - t.pK[c], nS = t.pS[c + 1] - t.pS[c];
                    for (int il = 0; il < nA; ++il)
                        for (int ks = 0; ks < nS; ++ks) { tflat.push_back((t.pA[c] + il) | ((t.pS[c] + ks) << 16)); tflat.push_back(vbase + il * nK); }
                    vbase += nA * nK;
                }
            }
        if ((rc = mem.up(tflat, &d_tflat))) return rc;
        ctx->db.tflat = d_tflat;
    }
    return TF_OK;
}

// the lists behind DBasis::kq_ptr .. kt_c belong to the build (mem): whoever releases them calls this
void EriBuild::forget_team_tables()
{
    ctx->db.kq_ptr = ctx->db.kq_off = ctx->db.kt_ptr = ctx->db.kt_k = nullptr; ctx->db.kt_c = nullptr;
}

// device index buffers sized for the largest possible slab, reused by every slab
int EriBuild::plan_index_buffers()
{
    int rc;
    size_t max_out = 0;
    for (int p : kets.mine_sorted) max_out = std::max<size_t>(max_out, (size_t)sto.pair_rows[p]);
    ix.cap_bra = std::min<size_t>(kets.mine_sorted.size(), 65535) + 1;
    ix.cap_out = (size_t)std::min<long long>(ctx->n_rows, slab.max_rows_c * 2 + (long long)max_out) + 1;
    // two sets of a slab's index lists: the lists of slab k + 1 are uploaded (on a stream of their own) while the kernels of slab k run;
    // the kernels themselves stay ordered by the streams (one half-transformed slab)
    ix.out_bytes = ix.cap_out * std::max(std::max(sizeof(OutRow), sizeof(OutRowP)), sizeof(OutRowT)); ix.rowcls_bytes = (size_t)slab.max_rows_c + 1;
    if ((rc = mem.alloc(&ix.d_bra, 2 * ix.cap_bra * sizeof(int)))) return rc;
    if ((rc = mem.alloc(&ix.d_braoff, 2 * ix.cap_bra * sizeof(long long)))) return rc;
    if (lt.use_team_pc) if ((rc = mem.alloc(&tt.d_brarec, 2 * ix.cap_bra * sizeof(BraRec)))) return rc;
    if ((rc = mem.alloc(&ix.d_out, 2 * ix.out_bytes))) return rc;
    if (sto.packed && !slab.per_class) if ((rc = mem.alloc(&ix.d_rowcls, 2 * ix.rowcls_bytes))) return rc;
    ix.d_bra_alloc = ix.d_bra; ix.d_braoff_alloc = ix.d_braoff; ix.d_out_alloc = ix.d_out;
    ix.d_brarec_alloc = tt.d_brarec; ix.d_rowcls_alloc = ix.d_rowcls;
    tt.d_bra_base = ix.d_bra;
    return TF_OK;
}

// Generation: slab size, work counters, ket lists and families, streams, the launch tables of the mode, the slabs' index lists
int EriBuild::plan_generation()
{
    int rc;
    if ((rc = plan_slab_size())) return rc;
    plan_work_counters();
    DBG("slab buffers allocated");
    slab.t_wall0 = std::chrono::steady_clock::now();
    if ((rc = plan_ket_lists()) || (rc = plan_ket_families())) return rc;
    // my bra pairs ordered by class: a slab is a run of that list, launches go per (bra class run, ket class)
    kets.mine_sorted.clear();
    for (int c = 0; c < sto.ncls; ++c)
        for (int p : ctx->class_pairs[c])
            if (sto.owner[p] == ctx->rank) kets.mine_sorted.push_back(p);
    if ((rc = setup_streams())) return rc;
    DBG("streams created");
    const bool team_ok = sto.packed && !EriKnobs::team_off() && bs.epool.size() < 0xffffffffull;
    lt.use_team_pc = team_ok && slab.per_class;                                        // per-class mode: eri_team_kernel for the uncontracted classes
    // (off by default: on the BASELINE basis sets eri_cfact_kernel is faster -- N2/cc-pVTZ 1.2 ms against 3.3-4.2 ms, Ar2/cc-pVQZ 18 ms against
    // 22-25 ms of ERI kernels: a team walks the primitive quartets of its shell quartet one after the other, a chain of dependent phases
    // with nothing else on the chip to hide it; TF_ERI_TEAMC=1 switches it on for experiments and for the parity tests)
    lt.use_teamc = team_ok && !slab.per_class && EriKnobs::teamc_on();                         // small-problem mode: eri_teamc_kernel over task lists
    lt.use_team = lt.use_team_pc || lt.use_teamc;                                       // the team kernels' tables are needed
    lt.teamc_pqmax = EriKnobs::teamc_pqmax();
    tt.kct.assign(sto.ncls, KClassTab());
    if (!slab.per_class) make_caps();
    DBG("stage: index-word tables");
    if ((rc = make_lrecs(!slab.per_class))) return rc;
    DBG("stage: team tables");
    if ((rc = plan_team_tables())) return rc;
    if (!slab.per_class)
        std::stable_sort(kets.mine_sorted.begin(), kets.mine_sorted.end(), [&](int x, int y) {
            const int gx = pair_group(x), gy = pair_group(y);
            return gx != gy ? gx < gy : pair_cost(x) > pair_cost(y);
        });
    if ((rc = plan_index_buffers())) return rc;
    DBG("stage: teamc tables");
    tc.tc_of.assign((size_t)sto.ncls * sto.ncls, -2);
    for (int p2 = 0; p2 < sto.npairs; ++p2) {
        tc.any_wide_pair = tc.any_wide_pair || bs.pairs[p2].La + bs.pairs[p2].Lb > TF_TEAM_LMAX;
        tc.max_npp_all = std::max(tc.max_npp_all, bs.pairs[p2].npp);
    }
    return TF_OK;
}

// ---- small-problem mode with team kernels (eri_teamc_kernel): class records per (bra class, ket class), created on demand; tasks
// per slab.  A quartet belongs to that kernel when both pair sums are <= TF_TEAM_LMAX and it has <= teamc_pqmax primitive quartets;
// eri_cfact_kernel skips exactly those (CFCaps::team_lmax / team_pqmax).
int EriBuild::teamc_class(int bcls, int kcls)
{
    int &slot = tc.tc_of[(size_t)bcls * sto.ncls + kcls];
    if (slot != -2) return slot;
    int maxblk, maxK, nnzc;
    TClass t = tclass_common(bcls, kcls, maxblk, maxK, nnzc);
    const int LAB = t.La + t.Lb, LCD = t.Lc + t.Ld;
    if (LAB > TF_TEAM_LMAX || LCD > TF_TEAM_LMAX) return slot = -1;
    const tfe::TeamSizes S = tfe::carve_teamc(t);
    const bool avail[3] = {eri_team_available(LAB, LCD, 16), eri_team_available(LAB, LCD, 64), eri_team_available(LAB, LCD, 256)};
    const int team = tfe::choose_team(avail, S.bytes, t.nT, nnzc, 52 * 1024, 96, 0);
    if (!team) return slot = -1;
    tc.tcs_host.push_back(t); tc.tc_team.push_back(team); tc.tc_lds.push_back(S.bytes[tfe::team_slot(team)]);
    return slot = (int)tc.tcs_host.size() - 1;
}

// small-problem mode with team kernels: the slab's tasks, one launch per (LAB, LCD, team, LDS size class)
int EriBuild::teamc_tasks(const std::vector<int> &bra, const std::vector<long long> &braoff, std::vector<TcLaunch> &tcl, bool &old_needed)
{
    int rc;
    std::map<std::array<int, 4>, int> lidx;
    int max_npp_bra = 1;
    for (size_t b = 0; b < bra.size(); ++b) {
        const int pb = bra[b], A = bs.pairs[pb].A, bcls = ctx->pair_class[pb];
        max_npp_bra = std::max(max_npp_bra, bs.pairs[pb].npp);
        for (int kc = 0; kc < sto.ncls; ++kc) {
            const std::vector<int> &kl = ctx->class_pairs[kc];
            const int nk_all = (int)(std::upper_bound(kl.begin(), kl.end(), A, [&](int a, int p2) { return a < bs.pairs[p2].A; }) - kl.begin());
            if (nk_all == 0) continue;
            const int id = teamc_class(bcls, kc);
            if (id < 0) continue;
            const int team = tc.tc_team[(size_t)id], NT = 256 / team;
            int lg = 10;
            while (((size_t)1 << lg) < tc.tc_lds[(size_t)id]) ++lg;
            const std::array<int, 4> key{tc.tcs_host[(size_t)id].La + tc.tcs_host[(size_t)id].Lb, tc.tcs_host[(size_t)id].Lc + tc.tcs_host[(size_t)id].Ld, team, lg};
            auto it = lidx.find(key);
            if (it == lidx.end()) { it = lidx.emplace(key, (int)tcl.size()).first; tcl.push_back(TcLaunch{key[0], key[1], team, 0, {}, {}}); }
            TcLaunch &TL = tcl[(size_t)it->second];
            TL.lds = std::max(TL.lds, tc.tc_lds[(size_t)id]);
            for (int g0 = 0; g0 < nk_all; g0 += NT) {
                const int nk = std::min(NT, nk_all - g0);
                int npq_max = 0, todo = 0;
                for (int u = 0; u < nk; ++u) {
                    const int npq = bs.pairs[pb].npp * bs.pairs[kl[(size_t)(g0 + u)]].npp;
                    if (npq <= lt.teamc_pqmax) { ++todo; npq_max = std::max(npq_max, npq); }
                }
                if (!todo) continue;                       // (every quartet of the group goes to eri_cfact_kernel)
                TL.tasks.push_back(TeamTask{id, pb, kets.ket_off[kc] + g0, nk, braoff[b]});
                TL.cost.push_back((double)npq_max * (tc.tcs_host[(size_t)id].nT + tc.tcs_host[(size_t)id].nacc));
            }
        }
    }
    old_needed = tc.any_wide_pair || (long long)max_npp_bra * tc.max_npp_all > lt.teamc_pqmax;
    // heaviest tasks first inside a launch (workgroups are dispatched in index order), all tasks in one device array
    std::vector<TeamTask> all;
    for (TcLaunch &TL : tcl) {
        std::vector<int> ord(TL.tasks.size());
        std::iota(ord.begin(), ord.end(), 0);
        std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return TL.cost[(size_t)x] > TL.cost[(size_t)y]; });
        std::vector<TeamTask> sorted(TL.tasks.size());
        for (size_t k = 0; k < ord.size(); ++k) sorted[k] = TL.tasks[(size_t)ord[k]];
        TL.tasks.swap(sorted);
        all.insert(all.end(), TL.tasks.begin(), TL.tasks.end());
    }
    if (tc.tcs_host.size() > tc.d_tcs_cap) {
        mem.blocks.release(tc.d_tcs);
        tc.d_tcs_cap = tc.tcs_host.size() + 64;
        if ((rc = mem.alloc(&tc.d_tcs, tc.d_tcs_cap * sizeof(TClass)))) return rc;
    }
    if (all.size() > tc.d_tasks_cap) {
        mem.blocks.release(tc.d_tasks);
        tc.d_tasks_cap = all.size() + 1024;
        if ((rc = mem.alloc(&tc.d_tasks, tc.d_tasks_cap * sizeof(TeamTask)))) return rc;
    }
    if (!tc.tcs_host.empty()) HIPCHK(ctx, hipMemcpy(tc.d_tcs, tc.tcs_host.data(), tc.tcs_host.size() * sizeof(TClass), hipMemcpyHostToDevice));
    if (!all.empty()) HIPCHK(ctx, hipMemcpy(tc.d_tasks, all.data(), all.size() * sizeof(TeamTask), hipMemcpyHostToDevice));
    return TF_OK;
}

int EriBuild::launch_teamc(const std::vector<TcLaunch> &tcl)
{
    int rc;
    // the team kernels write their quartets' part of the half-transformed slab (behind the ket transform of the others' part,
    // which has left zeros there); heaviest launches first, spread over the streams
    std::vector<size_t> first(tcl.size(), 0), order(tcl.size());
    for (size_t k = 1; k < tcl.size(); ++k) first[k] = first[k - 1] + tcl[k - 1].tasks.size();
    std::iota(order.begin(), order.end(), 0);
    auto total = [&](size_t k) { double c = 0; for (double x : tcl[k].cost) c += x; return c; };
    std::vector<double> tot(tcl.size());
    for (size_t k = 0; k < tcl.size(); ++k) tot[k] = total(k);
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return tot[x] > tot[y]; });
    hipEvent_t et[2];
    for (auto &e : et) { if ((rc = mem.event(&e))) return rc; ix.tev2.push_back(e); }
    HIPCHK(ctx, hipEventRecord(et[0], 0));
    HIPCHK(ctx, hipEventRecord(run.sev[0], 0));
    for (int k = 0; k < run.NSTREAM; ++k) HIPCHK(ctx, hipStreamWaitEvent(run.streams[k], run.sev[0], 0));
    int nl = 0;
    for (size_t k : order) {
        const TcLaunch &TL = tcl[k];
        if (TL.tasks.empty()) continue;
        TeamcLaunch a{TL.LAB, TL.LCD, TL.team, (unsigned)TL.tasks.size(), TL.lds, run.streams[nl++ % run.NSTREAM], &ctx->db, tc.d_tcs, tc.d_tasks + first[k], kets.d_kets,
                      lt.teamc_pqmax, slab.d_T2};
        const hipError_t e = eri_teamc_launch(a);
        if (e != hipSuccess && lt.team_error == hipSuccess) lt.team_error = e;
        count(TF_ERI_STAT_TEAMC);
        ++run.launch_count;
    }
    for (int k = 0; k < run.NSTREAM; ++k) {
        HIPCHK(ctx, hipEventRecord(run.sev[k], run.streams[k]));
        HIPCHK(ctx, hipStreamWaitEvent(0, run.sev[k], 0));
    }
    HIPCHK(ctx, hipEventRecord(et[1], 0));
    return TF_OK;
}

// a grid's y extent is at most 65535: fn(first, count) for every chunk of n rows
template <class F> static void grid_y_chunks(size_t n, F fn)
{
    for (size_t o0 = 0; o0 < n; o0 += 65535) fn(o0, (unsigned)std::min<size_t>(65535, n - o0));
}

// One pass of the slab loop: the next run of bra pairs that fits the slab, its index lists, its launches and transforms
int EriBuild::run_slab()
{
    int rc;
    std::vector<int> bra; std::vector<long long> braoff; std::vector<OutRow> outs;
    std::vector<OutRowP> outsP;
    std::vector<OutRowT> outsT;
    std::vector<signed char> rowcls;
    long long rows_c = 0;
    while (ix.cursor < kets.mine_sorted.size()) {
        const int p = kets.mine_sorted[ix.cursor];
        const tf::Shell &a = bs.shells[bs.pairs[p].A], &b = bs.shells[bs.pairs[p].B];
        const long long nr = (long long)a.ncomp * b.ncomp;
        if (!bra.empty() && (rows_c + nr > slab.cut_rows || bra.size() >= 65535 || outs.size() + outsP.size() + outsT.size() + (size_t)sto.pair_rows[p] >= ix.cap_out)) break;
        bra.push_back(p); braoff.push_back(rows_c);
        long long r = sto.rows.pair_first_row[p];
        for (int x = 0; x < out_dim(a); ++x)
            for (int y = 0; y < out_dim(b); ++y) {
                const int i = out_off(a) + x, j = out_off(b) + y;
                if (i < j) continue;
                if (!sto.packed) { outs.push_back(OutRow{i, j, a.cart_off, b.cart_off, b.ncomp, 0, rows_c, r++}); continue; }
                if (sto.tiles) { outsT.push_back(OutRowT{i, j, H.sigma[i], H.sigma[j], H.cls[i] ^ H.cls[j], b.ncomp, a.cart_off, b.cart_off, rows_c}); continue; }
                const int lr = sto.rows.rowmap[tfp::ikey(H.sigma[i], H.sigma[j])];
                OutRowP o{};
                o.i = i; o.j = j; o.iI = H.sigma[i]; o.lamj = H.loc[j]; o.c = H.cls[i] ^ H.cls[j]; o.ncb = b.ncomp;
                o.cartA = a.cart_off; o.cartB = b.cart_off;
                for (int t = 0; t < 4; ++t) o.secoff[t] = sto.rows.rowsec[6 * (size_t)lr + t];
                o.len = sto.rows.rowlen[lr]; o.slab_off = rows_c; o.ubase = sto.rows.rowoff[lr]; o.upos = sto.rows.rowsec[6 * (size_t)lr + 4]; o.unr = sto.rows.rowsec[6 * (size_t)lr + 5];
                outsP.push_back(o);
            }
        if (sto.packed && !slab.per_class)
            for (int ca = 0; ca < a.ncomp; ++ca)
                for (int cb = 0; cb < b.ncomp; ++cb) {
                    const int u = a.comp_off + ca, v = b.comp_off + cb;
                    rowcls.push_back((signed char)(((bs.c_lx[u] + bs.c_lx[v]) & 1) | (((bs.c_ly[u] + bs.c_ly[v]) & 1) << 1)));
                }
        rows_c += nr;
        const int Alim = sto.packed ? bs.pairs[p].A + 1 : sto.nsh;
        slab.n_quart += slab.cum_pairs[Alim];
        slab.n_primq += (long long)bs.pairs[p].npp * slab.cum_pp[Alim];
        slab.n_compq += nr * slab.cum_comp[Alim];
        {
            const double npp_ab = (double)bs.pairs[p].npp;
            const int lab = bs.pairs[p].La + bs.pairs[p].Lb;
            for (int c = 0; c < 4; ++c) {
                slab.nominal_flops += 8.0 * npp_ab * slab.pairW[p][c] * slab.cumW[Alim][c];
                for (int lcd = 0; lcd <= 10; ++lcd) {
                    const double L1 = (double)(lab + lcd + 1);
                    slab.nominal_flops += npp_ab * slab.pairNc[p][c] * slab.cumNL[Alim][4 * lcd + c] * (6.0 * L1 + 1.5 * L1 * L1 + 60.0);
                }
            }
        }
        ++ix.cursor;
    }
    // this set of index lists was last read by the kernels of the slab before the previous one: wait for that slab only
    const int set = (int)(ix.slab_no & 1);
    if (ix.slab_no >= 2) HIPCHK(ctx, hipEventSynchronize(ctx->bstr.slab_done(set)));
    ix.d_bra = ix.d_bra_alloc + (size_t)set * ix.cap_bra; ix.d_braoff = ix.d_braoff_alloc + (size_t)set * ix.cap_bra;
    ix.d_out = (char *)ix.d_out_alloc + (size_t)set * ix.out_bytes;
    if (ix.d_brarec_alloc) tt.d_brarec = ix.d_brarec_alloc + (size_t)set * ix.cap_bra;
    if (ix.d_rowcls_alloc) ix.d_rowcls = ix.d_rowcls_alloc + (size_t)set * ix.rowcls_bytes;
    tt.d_bra_base = ix.d_bra;
    ++ix.slab_no;
    ++run.stats[TF_ERI_STAT_SLABS];
    const hipStream_t cst = ctx->bstr.cstream();
    HIPCHK(ctx, hipMemcpyAsync(ix.d_bra, bra.data(), bra.size() * sizeof(int), hipMemcpyHostToDevice, cst));
    HIPCHK(ctx, hipMemcpyAsync(ix.d_braoff, braoff.data(), braoff.size() * sizeof(long long), hipMemcpyHostToDevice, cst));
    std::vector<BraRec> brec;
    if (lt.use_team_pc) {
        brec.resize(bra.size());
        for (size_t k = 0; k < bra.size(); ++k) {
            const tf::Pair &pr = bs.pairs[bra[k]];
            const double pp = bs.pp_p[pr.pp_off];
            brec[k] = BraRec{pp, bs.pp_Pz[pr.pp_off], bs.pp_K[pr.pp_off] / pp, (unsigned)pr.e_off, pr.A, braoff[k], 0};
        }
        HIPCHK(ctx, hipMemcpyAsync(tt.d_brarec, brec.data(), brec.size() * sizeof(BraRec), hipMemcpyHostToDevice, cst));
    }
    if (!outs.empty()) HIPCHK(ctx, hipMemcpyAsync(ix.d_out, outs.data(), outs.size() * sizeof(OutRow), hipMemcpyHostToDevice, cst));
    if (!outsP.empty()) HIPCHK(ctx, hipMemcpyAsync(ix.d_out, outsP.data(), outsP.size() * sizeof(OutRowP), hipMemcpyHostToDevice, cst));
    if (!outsT.empty()) HIPCHK(ctx, hipMemcpyAsync(ix.d_out, outsT.data(), outsT.size() * sizeof(OutRowT), hipMemcpyHostToDevice, cst));
    if (!rowcls.empty()) HIPCHK(ctx, hipMemcpyAsync(ix.d_rowcls, rowcls.data(), rowcls.size(), hipMemcpyHostToDevice, cst));
    HIPCHK(ctx, hipStreamSynchronize(cst));                // (pageable sources: the copies are complete; the host vectors may go)
    DBG("slab: %zu bra pairs, %lld cart rows, %zu out rows", bra.size(), rows_c, outs.size() + outsP.size() + outsT.size());
    hipEvent_t e4[4];
    for (auto &e : e4) { if ((rc = mem.event(&e))) return rc; ix.tev.push_back(e); }
    if (slab.per_class && !sto.packed && sto.ld != sto.N) HIPCHK(ctx, hipMemsetAsync(slab.d_T2, 0, (size_t)rows_c * sto.N * sto.ld * sizeof(double), 0));   // pad columns
    std::vector<TcLaunch> tcl;
    bool old_needed = !lt.use_teamc;
    if (lt.use_teamc && (rc = teamc_tasks(bra, braoff, tcl, old_needed))) return rc;
    // generic mode: eri_cfact_kernel stores only the components that are not zero by x/y parity
    if (!slab.per_class && old_needed) HIPCHK(ctx, hipMemsetAsync(slab.d_C, 0, (size_t)rows_c * sto.Nc * sto.Nc * sizeof(double), 0));
    HIPCHK(ctx, hipEventRecord(e4[0], 0));
    for (int k = 0; k < run.NSTREAM; ++k) HIPCHK(ctx, hipStreamWaitEvent(run.streams[k], e4[0], 0));
    // runs of equal bra class inside the slab
    size_t r0 = 0;
    if (!slab.per_class) { if (old_needed && (rc = launch_generic(bra, ix.d_bra, ix.d_braoff))) return rc; r0 = bra.size(); }
    while (r0 < bra.size()) {
        const int bcls = ctx->pair_class[bra[r0]];
        size_t r1 = r0;
        int max_npp = 1, Amax = 0;
        while (r1 < bra.size() && ctx->pair_class[bra[r1]] == bcls) {
            max_npp = std::max(max_npp, bs.pairs[bra[r1]].npp);
            Amax = std::max(Amax, bs.pairs[bra[r1]].A);
            ++r1;
        }
        for (int kcls = 0; kcls < sto.ncls; ++kcls)
            launch_class(bcls, kcls, max_npp, (unsigned)(r1 - r0), ix.d_bra + r0, ix.d_braoff + r0, Amax);
        r0 = r1;
    }
    for (int k = 0; k < run.NSTREAM; ++k) {
        HIPCHK(ctx, hipEventRecord(run.sev[k], run.streams[k]));
        HIPCHK(ctx, hipStreamWaitEvent(0, run.sev[k], 0));
    }
    HIPCHK(ctx, hipEventRecord(e4[1], 0));
    if (!slab.per_class && old_needed) {
        grid_y_chunks((size_t)rows_c, [&](size_t r0s, unsigned ny) {      // both ket axes in one pass over the slab
            if (sto.packed)
                hipLaunchKernelGGL(xform_ket_packed, dim3((unsigned)((sto.N + 3) / 4), ny), dim3(256), 0, 0, slab.d_C + (size_t)r0s * sto.Nc * sto.Nc,
                                   slab.d_T2 + (size_t)r0s * H.RLS, sto.Nc, ctx->bl, (long long)H.RLS, ix.d_rowcls + r0s, ctx->d_csr_ptr(), ctx->d_csr_idx(),
                                   ctx->d_csr_val());
            else
                hipLaunchKernelGGL(xform_ket_both, dim3((unsigned)((sto.N + 3) / 4), ny), dim3(256), 0, 0, slab.d_C + (size_t)r0s * sto.Nc * sto.Nc,
                                   slab.d_T2 + (size_t)r0s * sto.N * sto.ld, sto.Nc, sto.N, sto.ld, ctx->d_csr_ptr(), ctx->d_csr_idx(), ctx->d_csr_val(), 0);
        });
    }
    if (lt.use_teamc && !tcl.empty() && (rc = launch_teamc(tcl))) return rc;
    HIPCHK(ctx, hipEventRecord(e4[2], 0));
    if (!outs.empty()) {
        const unsigned gx = (unsigned)std::min<long long>((sto.row_len + 255) / 256, 4096);
        grid_y_chunks(outs.size(), [&](size_t o0, unsigned ny) {
            hipLaunchKernelGGL(xform_bra_store, dim3(gx, ny), dim3(256), 0, 0, slab.d_T2, ctx->d_eri(), reinterpret_cast<const OutRow *>(ix.d_out) + o0,
                               sto.row_len, ctx->d_csr_ptr(), ctx->d_csr_idx(), ctx->d_csr_val());
        });
    }
    if (!outsP.empty()) {
        int maxlen = 1;
        for (const OutRowP &o : outsP) maxlen = std::max(maxlen, o.len);
        grid_y_chunks(outsP.size(), [&](size_t o0, unsigned ny) {
            hipLaunchKernelGGL(xform_bra_store_packed, dim3((unsigned)((maxlen + 255) / 256), ny), dim3(256), 0, 0, slab.d_T2, ctx->d_eri(),
                               reinterpret_cast<const OutRowP *>(ix.d_out) + o0, (long long)H.RLS, ctx->bl, ctx->d_csr_ptr(), ctx->d_csr_idx(),
                               ctx->d_csr_val());
        });
    }
    if (!outsT.empty()) {
        grid_y_chunks(outsT.size(), [&](size_t o0, unsigned ny) {
            hipLaunchKernelGGL(xform_bra_store_tiles, dim3((unsigned)((H.RLS + 255) / 256), ny), dim3(256), 0, 0, slab.d_T2, ctx->d_eri(),
                               reinterpret_cast<const OutRowT *>(ix.d_out) + o0, (long long)H.RLS, ctx->bl, ctx->tv, ctx->d_csr_ptr(), ctx->d_csr_idx(),
                               ctx->d_csr_val());
        });
    }
    HIPCHK(ctx, hipEventRecord(e4[3], 0));
    HIPCHK(ctx, hipEventRecord(ctx->bstr.slab_done(set), 0));
    return TF_OK;
}

// Behind the last launch: drain the device, read the timing events, release the lists of the build, publish timings and counters
int EriBuild::finish()
{
    HIPCHK(ctx, hipDeviceSynchronize());
    DBG("device drained");
    HIPCHK(ctx, hipGetLastError());
    for (size_t k = 0; k + 3 < ix.tev.size(); k += 4) {
        slab.t_stage[1] += seconds_between(ix.tev[k], ix.tev[k + 1]);
        slab.t_stage[2] += seconds_between(ix.tev[k + 1], ix.tev[k + 2]);
        slab.t_stage[3] += seconds_between(ix.tev[k + 2], ix.tev[k + 3]);
    }
    for (size_t k = 0; k + 1 < ix.tev2.size(); k += 2) {
        const double dt = seconds_between(ix.tev2[k], ix.tev2[k + 1]);
        slab.t_stage[1] += dt; slab.t_stage[2] -= dt;
    }
    mem.release();
    forget_team_tables();
    if (lt.team_error != hipSuccess) TF_FAIL(ctx, TF_ENODEVICE, "launch of a team ERI kernel failed: %s", hipGetErrorString(lt.team_error));
    slab.t_stage[0] = std::chrono::duration<double>(std::chrono::steady_clock::now() - slab.t_wall0).count();
    std::copy(slab.t_stage, slab.t_stage + 4, ctx->eri_seconds);
    ctx->eri_counts[0] = slab.n_quart; ctx->eri_counts[1] = slab.n_primq; ctx->eri_counts[2] = slab.n_compq;
    ctx->eri_nominal_flops = slab.nominal_flops;
    std::copy(run.stats, run.stats + TF_ERI_STAT_COUNT, ctx->eri_stats);
    return TF_OK;
}

// Every way out of a build but the end of finish: launches may be in flight, so drain, then release the lists like finish does
void EriBuild::abandon()
{
    if (!mem.blocks.held.empty() || !mem.events.empty()) { (void)hipDeviceSynchronize(); mem.release(); }
    forget_team_tables();
}

}  // extern "C++"

// the units of a build in order; an error leaves the clean-up to the caller
static int eri_build_units(EriBuild &B)
{
    tf_ctx *ctx = B.ctx;
    int rc;
    if ((rc = B.plan_storage())) return rc;
    DBG("rows=%lld N=%d ld=%d (tensor + row tables allocated)", ctx->n_rows, B.sto.N, B.sto.ld);
    if ((rc = B.plan_generation())) return rc;
    DBG("stage: slab loop");
    while (B.ix.cursor < B.kets.mine_sorted.size())
        if ((rc = B.run_slab())) return rc;
    DBG("all slabs launched (%d class launches)", B.run.launch_count);
    // The tables only the CONSUMERS of the tensor need are built on the host while the generation kernels run
    if ((rc = B.upload_consumer_tables())) { (void)hipDeviceSynchronize(); return rc; }
    DBG("consumer tables built");
    if ((rc = B.finish())) return rc;
    DBG("scratch freed");
    if ((rc = B.alloc_jk_scratch())) return rc;
    DBG("build_eri done");
    ctx->have_eri = true;
    return TF_OK;
}

int tf_build_eri(tf_ctx *ctx, int spherical)
{
    if (!ctx) return TF_EINVAL;
    if (!ctx->have_basis) TF_FAIL(ctx, TF_EINVAL, "tf_build_eri: call tf_set_basis first");
    const tf::Basis &bs = ctx->bs;
    if (spherical && !bs.all_full)
        TF_FAIL(ctx, TF_EINVAL, "spherical output needs complete shells in canonical Cartesian order (use CARTHARM / spherical=0)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    free_eri(ctx);
    DBG("build_eri start");
    int rc = upload_csr(ctx, spherical);
    if (rc) return rc;
    DBG("csr uploaded");
    EriBuild B(ctx, spherical);
    if ((rc = eri_build_units(B))) B.abandon();
    return rc;
}

int tf_eri_storage(const tf_ctx *ctx, int64_t *bytes, int64_t *n_rows, int32_t *n, int32_t *ld)
{
    if (!ctx || !ctx->have_eri) return TF_EINVAL;
    if (bytes) *bytes = (int64_t)ctx->n_elems * (int64_t)sizeof(double);
    if (n_rows) *n_rows = ctx->n_rows;
    if (n) *n = ctx->N;
    if (ld) *ld = ctx->ld;
    return TF_OK;
}

int tf_set_eri_layout(tf_ctx *ctx, int layout)
{
    if (!ctx || layout < -1 || layout > 2) return TF_EINVAL;
    ctx->layout_req = layout;
    return TF_OK;
}

int tf_eri_layout(const tf_ctx *ctx) { return (ctx && ctx->have_eri) ? ctx->layout : TF_EINVAL; }
int tf_packed_pad(void) { return TF_TRI_PAD; }

int tf_eri_timings(const tf_ctx *ctx, double *s4)
{
    if (!ctx || !s4) return TF_EINVAL;
    std::copy(ctx->eri_seconds, ctx->eri_seconds + 4, s4);
    return TF_OK;
}

int tf_eri_counts(const tf_ctx *ctx, int64_t *c3)
{
    if (!ctx || !c3) return TF_EINVAL;
    for (int i = 0; i < 3; ++i) c3[i] = ctx->eri_counts[i];
    return TF_OK;
}

int tf_eri_build_stats(const tf_ctx *ctx, int64_t *out, int n)
{
    if (!ctx || !out || n < 0) return TF_EINVAL;
    for (int i = 0; i < n; ++i) out[i] = i < TF_ERI_STAT_COUNT ? ctx->eri_stats[i] : 0;
    return TF_OK;
}

int tf_eri_flops(const tf_ctx *ctx, double *nominal_flops)
{
    if (!ctx || !nominal_flops) return TF_EINVAL;
    *nominal_flops = ctx->eri_nominal_flops;
    return TF_OK;
}

int tf_segment_pad(void) { return TF_SEG_PAD; }

int tf_copy_eri(tf_ctx *ctx, double *host_out)
{
    if (!ctx) return TF_EINVAL;
    if (!ctx->have_eri || !host_out) TF_FAIL(ctx, TF_EINVAL, "tf_copy_eri: no tensor built / null output");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t total = (size_t)ctx->N * ctx->N * ctx->N * ctx->N;
    double *d_dense = nullptr;
    HIPCHK(ctx, tf_malloc((void **)&d_dense, total * sizeof(double)));
    const unsigned g = (unsigned)std::min<size_t>((total + 255) / 256, 1 << 20);
    if (ctx->layout == 2)
        hipLaunchKernelGGL(expand_dense_tiles_kernel, dim3(g), dim3(256), 0, 0, ctx->d_eri(), ctx->tv, ctx->bl, d_dense);
    else if (ctx->layout == 1)
        hipLaunchKernelGGL(expand_dense_packed_kernel, dim3(g), dim3(256), 0, 0, ctx->d_eri(), ctx->d_rowmap, ctx->d_rowoff, ctx->d_rowsec, ctx->bl, d_dense);
    else
        hipLaunchKernelGGL(expand_dense_kernel, dim3(g), dim3(256), 0, 0, ctx->d_eri(), ctx->d_rowmap, ctx->N, ctx->ld, d_dense);
    hipError_t e = hipMemcpy(host_out, d_dense, total * sizeof(double), hipMemcpyDeviceToHost);
    (void)tf_free(d_dense);
    HIPCHK(ctx, e);
    return TF_OK;
}

int tf_sample_eri(tf_ctx *ctx, int64_t n_idx, const int32_t *idx, double *values)
{
    if (!ctx) return TF_EINVAL;
    if (!ctx->have_eri || !idx || !values || n_idx < 0) TF_FAIL(ctx, TF_EINVAL, "tf_sample_eri: bad arguments");
    for (int64_t q = 0; q < 4 * n_idx; ++q)
        if (idx[q] < 0 || idx[q] >= ctx->N) TF_FAIL(ctx, TF_EINVAL, "tf_sample_eri: index out of range");
    if (n_idx == 0) return TF_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int *d_idx = nullptr; double *d_val = nullptr;
    HIPCHK(ctx, tf_malloc((void **)&d_idx, (size_t)n_idx * 4 * sizeof(int)));
    HIPCHK(ctx, tf_malloc((void **)&d_val, (size_t)n_idx * sizeof(double)));
    HIPCHK(ctx, hipMemcpy(d_idx, idx, (size_t)n_idx * 4 * sizeof(int), hipMemcpyHostToDevice));
    if (ctx->layout == 2)
        hipLaunchKernelGGL(sample_tiles_kernel, dim3((unsigned)((n_idx + 255) / 256)), dim3(256), 0, 0, ctx->d_eri(), ctx->tv, ctx->bl, (long long)n_idx, d_idx, d_val);
    else if (ctx->layout == 1)
        hipLaunchKernelGGL(sample_packed_kernel, dim3((unsigned)((n_idx + 255) / 256)), dim3(256), 0, 0, ctx->d_eri(), ctx->d_rowmap,
                           ctx->d_rowoff, ctx->d_rowsec, ctx->bl, (long long)n_idx, d_idx, d_val);
    else
        hipLaunchKernelGGL(sample_kernel, dim3((unsigned)((n_idx + 255) / 256)), dim3(256), 0, 0, ctx->d_eri(), ctx->d_rowmap, ctx->N,
                           ctx->ld, (long long)n_idx, d_idx, d_val);
    hipError_t e = hipMemcpy(values, d_val, (size_t)n_idx * sizeof(double), hipMemcpyDeviceToHost);
    (void)tf_free(d_idx); (void)tf_free(d_val);
    HIPCHK(ctx, e);
    return TF_OK;
}
