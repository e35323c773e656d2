// tf_scf_entry.hip.h -- the entry points of the eigensolver and of the native SCF cycles: tf_orthogonaliser,
// tf_diagonalise, tf_eigh_probe, the two counters, and tf_scf_rhf / _rhf_batch / _uhf / _uks with what they share (the J/K hook of a
// cycle, the guard of a sharded cycle, the lockstep rendezvous of a batch).  The cycles themselves are tf_scf.hip.h.  Included by
// tf_device.hip inside its extern "C" block, below every unit whose pieces the cycles call; one translation unit.

// The parity class of every output AO of the current build, offered to the eigensolvers of a workspace (tfscf::eigh_blocked verifies on
// every call that the matrix really has the block structure, so a vector that does not fit the problem only costs the test).
static void offer_symmetry(tf_ctx *ctx, tfscf::Workspace &w, int n)
{
    static const std::vector<int> none;
    tfscf::set_symmetry(w, (ctx->have_eri && (int)ctx->hl.cls.size() == n) ? ctx->hl.cls : none);
}

int tf_orthogonaliser(tf_ctx *ctx, int n, const double *S, double *X, double *S_inv, double *smallest_eig)
{
    if (!ctx) return TF_EINVAL;
    if (n < 1 || !S || !X) TF_FAIL(ctx, TF_EINVAL, "tf_orthogonaliser: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::string msg;
    offer_symmetry(ctx, ctx->scf, n);
    int rc = tfscf::orthogonaliser(ctx->scf, n, S, X, S_inv, smallest_eig, msg);
    if (rc) ctx->err = msg;
    return rc;
}

int tf_diagonalise(tf_ctx *ctx, int n, const double *F, const double *X, double *eps, double *C)
{
    if (!ctx) return TF_EINVAL;
    if (n < 1 || !F || !X || !eps || !C) TF_FAIL(ctx, TF_EINVAL, "tf_diagonalise: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::string msg;
    offer_symmetry(ctx, ctx->scf, n);
    int rc = tfscf::diagonalise(ctx->scf, n, F, X, eps, C, msg);
    if (rc) ctx->err = msg;
    return rc;
}

int tf_eigh_probe(tf_ctx *ctx, int n, int variant, int reps, double *seconds)
{
    if (!ctx || n < 1 || reps < 1 || !seconds) return TF_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::string msg;
    int rc = tfscf::eigh_probe(ctx->scf, n, variant, reps, seconds, msg);
    if (rc) ctx->err = msg;
    return rc;
}

int tf_jk_path_stats(tf_ctx *ctx, int64_t out[2])
{
    if (!ctx || !out) return TF_EINVAL;
    out[0] = ctx->jk_cd_passes; out[1] = ctx->jk_cd_declined;
    return TF_OK;
}

int tf_eigh_stats(tf_ctx *ctx, int64_t out[6])
{
    if (!ctx || !out) return TF_EINVAL;
    const tfscf::EigState &w = ctx->scf.eig;
    out[0] = w.ref_solves; out[1] = w.ref_steps; out[2] = w.ref_fallbacks; out[3] = w.sym_solves; out[4] = w.sym_declined;
    out[5] = w.jac_fallbacks;
    return TF_OK;
}

extern "C++" {
// A native cycle on a sharded tensor: every rank must take the same decisions from the same data.  For the duration of the cycle the
// control decisions are agreed over the ranks (agree_over_ranks) and rocBLAS runs without atomics (bitwise reproducible GEMMs; not
// otherwise: its split-K kernels need them -- the skinny GEMMs of the AO->MO transformation are ten times slower without).
struct ShardedCycleGuard {
    tf_ctx *ctx;
    bool on;
    explicit ShardedCycleGuard(tf_ctx *c) : ctx(c), on(c->world > 1 && (c->allreduce || c->comm)) {
        if (!on) { ctx->scf.agree = nullptr; return; }
        ctx->scf.agree = [c](const double *v, int nv, std::string &m) { return agree_over_ranks(c, v, nv, m); };
        if (ctx->scf.blas) (void)rocblas_set_atomics_mode(ctx->scf.blas, rocblas_atomics_not_allowed);
    }
    ~ShardedCycleGuard() {
        ctx->scf.agree = nullptr;
        if (on && ctx->scf.blas) (void)rocblas_set_atomics_mode(ctx->scf.blas, rocblas_atomics_allowed);
    }
};

// The J/K hook of the native cycles: J and K of the iteration's nd densities (1: restricted, 2: both spins in one fused pass),
// summed over the ranks of a sharded tensor
static int cycle_jk(tf_ctx *ctx, int nd, const double *dPa, const double *dPb, double *dJa, double *dJb, double *dKa, double *dKb, hipStream_t st)
{
    const double *p[2] = {dPa, dPb};
    double *j[2] = {dJa, dJb}, *k[2] = {dKa, dKb};
    int rcj = launch_jk(ctx, nd, p, j, k, st, nullptr, true);       // (a cycle's densities are class-diagonal unless a field along x / y mixes the classes)
    return rcj ? rcj : allreduce_jk(ctx, nd, j, k, st);
}

// The argument checks tf_scf_uhf and tf_scf_uks share, under the entry point's name
static int unrestricted_checks(tf_ctx *ctx, const char *who, const tf_scf_opts *opts, const double *S, const double *T, const double *V,
                               const double *P0_alpha, const double *P0_beta, int n_alpha, int n_beta, const tf_scf_uhf_result *out)
{
    if (!ctx) return TF_EINVAL;
    if (!ctx->have_eri) TF_FAIL(ctx, TF_EINVAL, "%s: call tf_build_eri first", who);
    if (!opts || !S || !T || !V || !P0_alpha || !P0_beta || !out || n_alpha < 1 || n_alpha > ctx->N || n_beta < 0 || n_beta > n_alpha)
        TF_FAIL(ctx, TF_EINVAL, "%s: bad arguments", who);
    return TF_OK;
}

// What tf_scf_uhf and tf_scf_uks do alike once each has checked its arguments; xc empty for Hartree-Fock (its failures go to msg)
static int scf_unrestricted(tf_ctx *ctx, const tf_scf_opts *opts, const double *S, const double *T, const double *V, const double *Fext,
                            const double *X, const double *P0_alpha, const double *P0_beta, double E0, int n_alpha, int n_beta, double V_NN,
                            tf_scf_uhf_result *out, std::string &msg, const tfscf::XC2Fn &xc)
{
    auto jk2 = [&](const double *dPa, const double *dPb, double *dJa, double *dJb, double *dKa, double *dKb, hipStream_t st) {
        return cycle_jk(ctx, 2, dPa, dPb, dJa, dJb, dKa, dKb, st);
    };
    tfscf::UhfOut uo;
    for (int sp = 0; sp < 2; ++sp) { uo.P[sp] = out->P_spin[sp]; uo.C[sp] = out->C_spin[sp]; uo.eps[sp] = out->eps_spin[sp]; uo.F[sp] = out->F_spin[sp]; }
    ShardedCycleGuard guard(ctx);
    offer_symmetry(ctx, ctx->scf, ctx->N);
    int rc = tfscf::run_uhf(ctx->scf, ctx->N, *opts, S, T, V, Fext, X, P0_alpha, P0_beta, E0, n_alpha, n_beta, V_NN, jk2, out->common, uo, msg, xc);
    if (rc && !msg.empty()) ctx->err = msg;
    return rc;
}
}

int tf_scf_rhf(tf_ctx *ctx, const tf_scf_opts *opts, const double *S, const double *T, const double *V, const double *Fext,
               const double *X, const double *P0, double E0, int n_occ, double V_NN, tf_scf_result *out)
{
    if (!ctx) return TF_EINVAL;
    if (!ctx->have_eri) TF_FAIL(ctx, TF_EINVAL, "tf_scf_rhf: call tf_build_eri first");
    if (!opts || !S || !T || !V || !P0 || !out || n_occ < 1 || n_occ > ctx->N) TF_FAIL(ctx, TF_EINVAL, "tf_scf_rhf: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::string msg;
    auto jk = [&](const double *dP, double *dJ, double *dK, hipStream_t st) { return cycle_jk(ctx, 1, dP, dP, dJ, dJ, dK, dK, st); };
    tfscf::XCFn xc;
    if (ctx->grid.G > 0) {
        const int rc = dft_grid_checks(ctx, "tf_scf_rhf", "", true);
        if (rc) return rc;
        xc = [&](const double *dP, double *dV, double *o3) { return tfdft::vxc(ctx->scf.blas, ctx->grid, dP, dV, o3, msg); };
    }
    ShardedCycleGuard guard(ctx);
    offer_symmetry(ctx, ctx->scf, ctx->N);
    int rc = tfscf::run_rhf(ctx->scf, ctx->N, *opts, S, T, V, Fext, X, P0, E0, n_occ, V_NN, jk, *out, msg, xc);
    if (rc && !msg.empty()) ctx->err = msg;
    return rc;
}

extern "C++" {
// Rendezvous of the cycles of a lockstep batch in their Fock builds (tf_scf_rhf_batch): every cycle runs the unmodified native cycle
// (tfscf::run_rhf) on a host thread of its own and asks for J and K of its density once per iteration; the last cycle to arrive sends
// the densities of all cycles still iterating through the tensor together (two per pass, jk_packed_kernel<2>).
struct LockstepJK {
    struct Req { const double *dP; double *dJ, *dK; };
    tf_ctx *ctx;
    std::mutex mu;
    std::condition_variable cv;
    int active = 0, waiting = 0, last_rc = TF_OK;
    long long generation = 0, passes = 0, builds = 0;
    std::vector<Req> req;
    hipEvent_t ev[2] = {nullptr, nullptr};          // "the builds of generation g are queued", alternating
    LockstepJK(tf_ctx *c, int n) : ctx(c), active(n), req((size_t)n)
    {
        (void)hipEventCreateWithFlags(&ev[0], hipEventDisableTiming);
        (void)hipEventCreateWithFlags(&ev[1], hipEventDisableTiming);
    }
    ~LockstepJK() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    void build_locked(hipStream_t st)               // on the stream of the cycle that arrived last; the others wait for its event
    {
        int rc = TF_OK;
        const int cap = ctx->layout == 2 ? 8 : 2;   // densities per pass over the tensor: the tiles layout's wide pass takes eight, the packed kernel two
        for (int q = 0; q < waiting && rc == TF_OK; q += cap) {
            const int nd = std::min(cap, waiting - q);
            const double *p[8];
            double *j[8], *k[8];
            for (int d = 0; d < nd; ++d) { p[d] = req[q + d].dP; j[d] = req[q + d].dJ; k[d] = req[q + d].dK; }
            rc = launch_jk(ctx, nd, p, j, k, st, nullptr, true);
            ++passes; builds += nd;
        }
        if (hipEventRecord(ev[generation & 1], st) != hipSuccess && rc == TF_OK) rc = TF_ENODEVICE;
        last_rc = rc;
        waiting = 0;
        ++generation;
        cv.notify_all();
    }
    int fock(const double *dP, double *dJ, double *dK, hipStream_t st)
    {
        if (hipStreamSynchronize(st) != hipSuccess) return TF_ENODEVICE;   // this cycle's density is complete before another stream reads it
        hipEvent_t done;
        int rc;
        {
            std::unique_lock<std::mutex> lk(mu);
            req[(size_t)waiting++] = Req{dP, dJ, dK};
            const long long g = generation;
            if (waiting == active) build_locked(st);
            else cv.wait(lk, [&] { return generation != g; });
            done = ev[g & 1];
            rc = last_rc;
        }
        if (hipStreamWaitEvent(st, done, 0) != hipSuccess && rc == TF_OK) rc = TF_ENODEVICE;
        return rc;
    }
    void finish(hipStream_t st)                     // a cycle has left its loop: those waiting may be complete now
    {
        std::unique_lock<std::mutex> lk(mu);
        --active;
        if (active > 0 && waiting == active) build_locked(st);
    }
};
}

int tf_scf_rhf_batch(tf_ctx *ctx, int n_cycles, const tf_scf_opts *opts, const double *S, const double *T, const double *V,
                     const double *const *Fext, const double *X, const double *const *P0, const double *E0, int n_occ, double V_NN,
                     tf_scf_result *out, int32_t *rc_out, int64_t *passes_out)
{
    if (!ctx) return TF_EINVAL;
    if (!ctx->have_eri) TF_FAIL(ctx, TF_EINVAL, "tf_scf_rhf_batch: call tf_build_eri first");
    if (n_cycles < 1 || n_cycles > 64 || !opts || !S || !T || !V || !P0 || !E0 || !out || n_occ < 1 || n_occ > ctx->N)
        TF_FAIL(ctx, TF_EINVAL, "tf_scf_rhf_batch: bad arguments");
    if (ctx->world > 1) TF_FAIL(ctx, TF_EINVAL, "tf_scf_rhf_batch: lockstep batches run on an unsharded tensor (world = 1) in this build");
    if (ctx->grid.G > 0) TF_FAIL(ctx, TF_EINVAL, "tf_scf_rhf_batch: lockstep batches run Hartree-Fock cycles (clear the DFT grid with tf_dft_clear)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    while ((int)ctx->scf_batch.size() < n_cycles) ctx->scf_batch.emplace_back(new tfscf::Workspace());
    LockstepJK ls(ctx, n_cycles);
    static const bool serial_streams = getenv("TF_BATCH_ONE_STREAM") != nullptr;      // (A/B: every cycle on the legacy default stream)
    std::vector<int> rcs((size_t)n_cycles, TF_OK);
    std::vector<std::string> msgs((size_t)n_cycles);
    std::vector<std::thread> threads;
    // At most TF_BATCH_STREAMS (4) streams for the cycles, shared round-robin: the O(N^3) steps of four cycles side by side fill the chip;
    // more of them at once only slow each other down.  (A stream per cycle was the same thing while the process had 4 hardware queues; with
    // the 16 the tensor build wants, eight truly concurrent cycles took 0.94 s for the N = 400 polarisability instead of 0.58 s.)
    static const int batch_streams = getenv("TF_BATCH_STREAMS") ? std::max(1, atoi(getenv("TF_BATCH_STREAMS"))) : 4;
    std::vector<hipStream_t> pool((size_t)std::min(n_cycles, batch_streams), nullptr);
    if (!serial_streams)
        for (auto &ps : pool)
            if (hipStreamCreateWithFlags(&ps, hipStreamNonBlocking) != hipSuccess) ps = nullptr;
    for (int c = 0; c < n_cycles; ++c)
        threads.emplace_back([&, c] {
            // a host thread per cycle on one of the pool's non-blocking streams: the O(N^3) steps of different cycles overlap on the device
            (void)hipSetDevice(ctx->device);
            hipStream_t st = serial_streams ? nullptr : pool[(size_t)c % pool.size()];
            tfscf::t_stream = st;
            auto jk = [&](const double *dP, double *dJ, double *dK, hipStream_t s2) { return ls.fock(dP, dJ, dK, s2); };
            offer_symmetry(ctx, *ctx->scf_batch[(size_t)c], ctx->N);
            rcs[(size_t)c] = tfscf::run_rhf(*ctx->scf_batch[(size_t)c], ctx->N, *opts, S, T, V, Fext ? Fext[c] : nullptr, X, P0[c], E0[c], n_occ, V_NN, jk,
                                             out[c], msgs[(size_t)c], tfscf::XCFn());
            (void)hipStreamSynchronize(st);
            ls.finish(st);
            (void)hipStreamSynchronize(st);
            tfscf::t_stream = nullptr;
        });
    for (auto &t : threads) t.join();
    for (hipStream_t ps : pool)
        if (ps) (void)hipStreamDestroy(ps);
    int rc = TF_OK;
    for (int c = 0; c < n_cycles; ++c) {
        if (rc_out) rc_out[c] = rcs[(size_t)c];
        if (rcs[(size_t)c] != TF_OK && rc == TF_OK) { rc = rcs[(size_t)c]; ctx->err = "cycle " + std::to_string(c) + ": " + msgs[(size_t)c]; }
    }
    if (passes_out) { passes_out[0] = ls.passes; passes_out[1] = ls.builds; }
    return rc;
}

int tf_scf_uhf(tf_ctx *ctx, const tf_scf_opts *opts, const double *S, const double *T, const double *V, const double *Fext,
               const double *X, const double *P0_alpha, const double *P0_beta, double E0, int n_alpha, int n_beta, double V_NN,
               tf_scf_uhf_result *out)
{
    if (const int bad = unrestricted_checks(ctx, "tf_scf_uhf", opts, S, T, V, P0_alpha, P0_beta, n_alpha, n_beta, out)) return bad;
    if (ctx->grid.G > 0)
        TF_FAIL(ctx, TF_EINVAL, "tf_scf_uhf: unrestricted Kohn-Sham is not implemented by the Hartree-Fock entry point (call tf_scf_uks, or tf_dft_clear)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::string msg;
    return scf_unrestricted(ctx, opts, S, T, V, Fext, X, P0_alpha, P0_beta, E0, n_alpha, n_beta, V_NN, out, msg, tfscf::XC2Fn());
}

int tf_scf_uks(tf_ctx *ctx, const tf_scf_opts *opts, const double *S, const double *T, const double *V, const double *Fext,
               const double *X, const double *P0_alpha, const double *P0_beta, double E0, int n_alpha, int n_beta, double V_NN,
               tf_scf_uhf_result *out)
{
    if (const int bad = unrestricted_checks(ctx, "tf_scf_uks", opts, S, T, V, P0_alpha, P0_beta, n_alpha, n_beta, out)) return bad;
    const int rc = dft_grid_checks(ctx, "tf_scf_uks", " (unrestricted Hartree-Fock is tf_scf_uhf)", true);
    if (rc) return rc;
    if (ctx->world > 1) TF_FAIL(ctx, TF_EINVAL, "tf_scf_uks: unrestricted Kohn-Sham runs on an unsharded tensor (world = 1) in this build");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::string msg;
    tfscf::XC2Fn xc = [&](const double *dPa, const double *dPb, double *dVa, double *dVb, double *o5) {
        return tfdft::vxc_unrestricted(ctx->scf.blas, ctx->grid, dPa, dPb, dVa, dVb, o5, msg);
    };
    return scf_unrestricted(ctx, opts, S, T, V, Fext, X, P0_alpha, P0_beta, E0, n_alpha, n_beta, V_NN, out, msg, xc);
}
