// tf_corr_host.hip.h -- the host drivers of the correlated methods: the AO->MO transformation, RMP2 / UMP2, MP3, MP4, LCCD / CCD,
// LCCSD / QCISD / CCSD, the perturbative triples, the MP2 density and the ladder probe.  Included by tf_device.hip (one translation unit:
// struct tf_ctx, tf_malloc, launch_jk, TF_FAIL and HIPCHK are defined there, above the include); the kernels are in tf_mp2.hip.h ...
// tf_mp2dens.hip.h.  First the pieces the drivers share (also with tf_excited_host.hip.h, included after this file), then the drivers.
// who uses what; every driver keeps its order of launches, rocBLAS calls and copies on the null stream, and of its host sums.
#pragma once
#include "tf_cc_diis.h"

// ---- shared pieces ----------------------------------------------------------------------------------------------------------------

static const int CORR_NBLK = 1024;     // blocks of the energy and update kernels: their partials are summed in block order

// (DeviceBlocks, the owner of the device allocations of one call -- freed on every return path -- is defined in tf_ctx.hip.h)

// "set ctx->err, return the code"; m may be ctx->err itself (a callee's message passed on)
static int corr_fail(tf_ctx *ctx, int code, const std::string &m)
{
    if (&m != &ctx->err) ctx->err = m;
    return code;
}

// rocBLAS without atomics for this scope (split-K kernels would change their sums from run to run); the previous mode comes back on
// every exit
struct __attribute__((visibility("hidden"))) BlasAtomicsOff {
    rocblas_handle blas;
    rocblas_atomics_mode mode = rocblas_atomics_allowed;
    bool set = false;
    explicit BlasAtomicsOff(rocblas_handle h) : blas(h)
    {
        set = rocblas_get_atomics_mode(blas, &mode) == rocblas_status_success &&
              rocblas_set_atomics_mode(blas, rocblas_atomics_not_allowed) == rocblas_status_success;
    }
    BlasAtomicsOff(const BlasAtomicsOff &) = delete;
    BlasAtomicsOff &operator=(const BlasAtomicsOff &) = delete;
    ~BlasAtomicsOff() { if (set) (void)rocblas_set_atomics_mode(blas, mode); }
};

// One check for every rocBLAS / rocSOLVER call of the drivers; needs ctx and who in scope
#define CORR_BLAS_WHAT(what, call) do { if ((call) != rocblas_status_success) return corr_fail(ctx, TF_ELINALG, std::string(who) + ": " what " failed: " #call); } while (0)
#define CORR_BLAS(call) CORR_BLAS_WHAT("rocBLAS", call)

// (sum_partials_host, the host sum of the blocks' partials in block order, is defined in tf_ctx.hip.h: the Kohn-Sham path uses it too)

// launch_jk for nd <= 8 general (non-symmetric) densities P [nd][N][N] with J and K [nd][N][N]: all eight argument slots filled, the
// slots past nd repeating the last density
static int launch_jk_general(tf_ctx *ctx, int nd, const double *P, double *J, double *K)
{
    const JkSlots s(nd, (size_t)ctx->N * ctx->N, P, J, K);
    const int nonsym[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    return launch_jk(ctx, nd, s.p, s.j, s.k, 0, nonsym);
}

static std::chrono::steady_clock::time_point corr_stamp() { (void)hipDeviceSynchronize(); return std::chrono::steady_clock::now(); }
static double corr_secs(std::chrono::steady_clock::duration d) { return std::chrono::duration<double>(d).count(); }
// seconds[0..3] of a driver with three consecutive stages: the wall time t0 .. t3, then the stages t0 .. t1, t1 .. t2, t2 .. t3
using CorrTime = std::chrono::steady_clock::time_point;
static void corr_stage_seconds(double *seconds, CorrTime t0, CorrTime t1, CorrTime t2, CorrTime t3)
{
    seconds[0] = corr_secs(t3 - t0); seconds[1] = corr_secs(t1 - t0); seconds[2] = corr_secs(t2 - t1); seconds[3] = corr_secs(t3 - t2);
}

// out [N][n] = the columns [first, first + n) of C [N][ld]
static void column_window(const double *C, int N, int ld, int first, int n, double *out)
{
    for (int m = 0; m < N; ++m)
        for (int i = 0; i < n; ++i) out[(size_t)m * n + i] = C[(size_t)m * ld + first + i];
}

// The prologue of a driver on restricted orbitals: sizes, the occupied window [n_frozen, n_occ) and the virtual window [n_occ, N) of C,
// and (corr_upload) eps, C_v, C_o on the device, on the packed layout also in the internal AO order of the ladder (corr_permute)
struct __attribute__((visibility("hidden"))) CorrSetup {
    int N = 0, n_occ = 0, n_frozen = 0, o = 0, v = 0;
    long long ov = 0, B2 = 0;                                 // o v and (o v)^2
    bool packed = false;                                      // the AO-direct ladder kernel; rows / tiles: the exchange build
    std::vector<double> Co, Cv;                               // [N][o], [N][v]
    std::chrono::steady_clock::time_point t0;
    double *d_eps = nullptr, *d_Cv = nullptr, *d_Cvi = nullptr, *d_Co = nullptr, *d_Coi = nullptr;
    const double *Cvl = nullptr, *Col = nullptr;              // C_v, C_o in the AO order of the ladder's T and Z
    void windows(int N_, int n_occ_, int n_frozen_, const double *C)
    {
        N = N_; n_occ = n_occ_; n_frozen = n_frozen_; o = n_occ - n_frozen; v = N - n_occ;
        ov = (long long)o * v; B2 = ov * ov;
        Co.resize((size_t)N * o); Cv.resize((size_t)N * v);
        column_window(C, N, N, n_frozen, o, Co.data());
        column_window(C, N, N, n_occ, v, Cv.data());
    }
};

// The checks every driver starts with; needs = what the driver's "bad arguments" message adds (may be empty)
static int corr_args(tf_ctx *ctx, const char *who, bool pointers_ok, const char *needs, int n_occ, int n_frozen)
{
    if (!ctx) return TF_EINVAL;
    if (!ctx->have_eri) TF_FAIL(ctx, TF_EINVAL, "%s: call tf_build_eri first", who);
    if (!pointers_ok || n_frozen < 0 || n_occ <= n_frozen || n_occ >= ctx->N) TF_FAIL(ctx, TF_EINVAL, "%s: bad arguments%s", who, needs);
    return TF_OK;
}

// After the driver's own checks: one rank only, the device, the start of the clock, the SCF work space, the windows
static int corr_begin(tf_ctx *ctx, const char *who, int n_occ, int n_frozen, const double *C, CorrSetup &S)
{
    if (ctx->world > 1) TF_FAIL(ctx, TF_EINVAL, "%s: a sharded tensor (world > 1) is not supported", who);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    S.t0 = std::chrono::steady_clock::now();
    std::string msg;
    const int rc = tfscf::ensure(ctx->scf, ctx->N, 6, msg);
    if (rc) { ctx->err = msg; return rc; }
    S.packed = ctx->layout == 1;
    S.windows(ctx->N, n_occ, n_frozen, C);
    return TF_OK;
}

// eps -> d_eps (the driver's, or N doubles of mem's when null), C_v and -- with_Co -- C_o, each with a second buffer for corr_permute
static int corr_upload(tf_ctx *ctx, const char *who, CorrSetup &S, DeviceBlocks &mem, const double *eps, double *d_eps, bool with_Co,
                       const std::string &oom)
{
    const size_t nv = (size_t)S.N * S.v, no = (size_t)S.N * S.o;
    S.d_eps = d_eps ? d_eps : mem.alloc((size_t)S.N);
    S.d_Cv = mem.alloc(nv); S.d_Cvi = mem.alloc(nv);
    if (with_Co) { S.d_Co = mem.alloc(no); S.d_Coi = mem.alloc(no); }
    if (!S.d_eps || !S.d_Cv || !S.d_Cvi || (with_Co && (!S.d_Co || !S.d_Coi))) return corr_fail(ctx, TF_ENOMEM, oom);
    if (hipMemcpy(S.d_eps, eps, (size_t)S.N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(S.d_Cv, S.Cv.data(), nv * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        (with_Co && hipMemcpy(S.d_Co, S.Co.data(), no * sizeof(double), hipMemcpyHostToDevice) != hipSuccess))
        return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": copy failed");
    S.Cvl = S.d_Cv; S.Col = S.d_Co;
    return TF_OK;
}

// Packed layout: the coefficients' rows in the internal AO order (null stream), which Cvl / Col then name
static void corr_permute(tf_ctx *ctx, CorrSetup &S)
{
    if (!S.packed) return;
    const int N = S.N;
    hipLaunchKernelGGL(tfmp2::permute_rows_kernel, dim3((unsigned)((N * S.v + 255) / 256)), dim3(256), 0, 0, S.d_Cv, ctx->bl.origI, N, S.v, S.d_Cvi);
    S.Cvl = S.d_Cvi;
    if (S.d_Co) {
        hipLaunchKernelGGL(tfmp2::permute_rows_kernel, dim3((unsigned)((N * S.o + 255) / 256)), dim3(256), 0, 0, S.d_Co, ctx->bl.origI, N, S.o, S.d_Coi);
        S.Col = S.d_Coi;
    }
}

// The work space of the short-index-first transformations, kept by the context: grown when a call needs more.  false: out of memory
static bool grow_mo_pool(tf_ctx *ctx, size_t need)
{
    if (ctx->blk.ensure(CB_MO_POOL, need) != 0) { (void)hipGetLastError(); return false; }
    return true;
}

// ---- AO->MO transformation and RMP2 (next row of the hot path: consumers of the resident tensor) ----------------------

// *d_out (owner's) = (C1 C2|C3 C4) [n1][n2][n3][n4] on the device.  On failure *d_out is null and nothing is left allocated.
static int mo_transform_device(tf_ctx *ctx, const double *C1, int n1, const double *C2, int n2, const double *C3, int n3, const double *C4,
                               int n4, DeviceBlocks &owner, double **d_out, double *seconds)
{
    const int N = ctx->N;
    *d_out = nullptr;
    std::string msg;
    int rc = tfscf::ensure(ctx->scf, N, 6, msg);
    if (rc) { ctx->err = msg; return rc; }
    if (ctx->world > 1 && !ctx->allreduce && !ctx->comm)
        TF_FAIL(ctx, TF_EINVAL, "AO->MO transformation of a sharded tensor (world > 1) needs an RCCL communicator (tf_comm_init) or the all-reduce hook (tf_set_allreduce)");
    const bool packed = ctx->layout >= 1, tiles = ctx->layout == 2;
    DeviceBlocks tmp;
    double *dC[4] = {nullptr, nullptr, nullptr, nullptr}, *dG[2] = {nullptr, nullptr};
    const double *hC[4] = {C1, C2, C3, C4};
    const int nk[4] = {n1, n2, n3, n4};
    const size_t total = (size_t)n1 * n2 * n3 * n4;
    // packed rows hold the pairs (kl) <= (ij): out[pq][rs] = G(C1 C2 C3 C4)[pq][rs] + G(C3 C4 C1 C2)[rs][pq]; one transformation
    // serves both terms when the two coefficient pairs are the same matrices ((ia|jb), (pq|rs) with one C)
    const bool same_pairs = n1 == n3 && n2 == n4 && std::memcmp(C1, C3, (size_t)N * n1 * sizeof(double)) == 0 &&
                            std::memcmp(C2, C4, (size_t)N * n2 * sizeof(double)) == 0;
    double secs = 0.0;
    auto fail = [&](int code, const std::string &m) { owner.release(*d_out); *d_out = nullptr; return corr_fail(ctx, code, m); };
    for (int k = 0; k < 4; ++k) {
        if (!(dC[k] = tmp.alloc((size_t)N * nk[k]))) return fail(TF_ENOMEM, "AO->MO transformation: out of device memory");
        if (hipMemcpy(dC[k], hC[k], (size_t)N * nk[k] * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return fail(TF_ENODEVICE, "AO->MO transformation: copy failed");
    }
    if (!(*d_out = owner.alloc(total + 1))) return fail(TF_ENOMEM, "AO->MO transformation: out of device memory");   // (+ 1: the status word of the hook's exchange)
    // the short index first: a ket coefficient matrix of at most 32 columns (the occupied orbitals of (ia|jb)) goes through the hand-written
    // first quarter on the packed segments (tfmp2::mo_q1_kernel); TF_MO_Q1=0 keeps the expanded-block path (A/B, tests)
    const char *q1env = getenv("TF_MO_Q1");
    const bool q1_allowed = packed && !tiles && !(q1env && q1env[0] == '0');
    auto run = [&](int a, int b, int c, int d, double *dst) {
        double s1 = 0.0;
        if (q1_allowed && nk[c] <= 32 && nk[a] <= 32 && (size_t)N * ((nk[a] + 1) & ~1) * sizeof(double) + (size_t)N * sizeof(int) <= ((size_t)150 << 10)) {
            const size_t need = tfmp2::q1_pool_doubles(N, ctx->n_rows, nk[a], nk[b], nk[c], nk[d]) * sizeof(double);
            size_t free_b = 0, total_b = 0;
            const bool fits = need <= ctx->blk.cap[CB_MO_POOL] || (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need + ((size_t)2 << 30) <= free_b + ctx->blk.cap[CB_MO_POOL] + tfcache::cached());
            if (fits && grow_mo_pool(ctx, need)) {
                int r = tfmp2::transform_q1(ctx->scf.blas, ctx->d_eri(), ctx->d_rowoff, ctx->d_rowsec, ctx->bl, ctx->d_row_ij, ctx->d_rowmap, ctx->n_rows, N,
                                            dC[a], nk[a], dC[b], nk[b], dC[c], nk[c], dC[d], nk[d], dst, ctx->mo_pool(), &s1, msg);
                secs += s1;
                return r;
            }
        }
        tfmp2::PackedRows pr{};
        if (packed) {
            for (int q = 0; q < 4; ++q) { pr.csize[q] = ctx->hl.csize[q]; pr.cstart[q] = ctx->hl.cstart[q]; pr.NP[q] = ctx->hl.NP[q]; }
            for (int q = 0; q < 5; ++q) pr.class_row_off[q] = ctx->class_row_off[q];
            pr.d_class_rows = ctx->d_class_rows; pr.d_row_pos = ctx->d_row_pos;
        }
        int r = tfmp2::transform(ctx->scf.blas, ctx->d_eri(), ctx->d_rowmap, (packed && !tiles) ? ctx->d_rowoff : nullptr, ctx->d_rowsec, ctx->bl, pr,
                                 ctx->d_row_ij, ctx->n_rows, N, ctx->ld, dC[a], nk[a], dC[b], nk[b], dC[c], nk[c], dC[d], nk[d], dst, &s1, msg,
                                 tiles ? &ctx->tv : nullptr);
        secs += s1;
        return r;
    };
    if (!packed) {
        if ((rc = run(0, 1, 2, 3, *d_out))) return fail(rc, msg);
    } else {
        if (!(dG[0] = tmp.alloc(total))) return fail(TF_ENOMEM, "AO->MO transformation: out of device memory");
        if ((rc = run(0, 1, 2, 3, dG[0]))) return fail(rc, msg);
        if (!same_pairs) {
            if (!(dG[1] = tmp.alloc(total))) return fail(TF_ENOMEM, "AO->MO transformation: out of device memory");
            if ((rc = run(2, 3, 0, 1, dG[1]))) return fail(rc, msg);
        }
        const long long A = (long long)n1 * n2, B = (long long)n3 * n4;
        hipLaunchKernelGGL(add_transposed_kernel, dim3((unsigned)((B + 31) / 32), (unsigned)((A + 31) / 32)), dim3(32, 8), 0, 0, dG[0],
                           same_pairs ? dG[0] : dG[1], A, B, *d_out);
        if (hipGetLastError() != hipSuccess) return fail(TF_ENODEVICE, "AO->MO transformation: launch failed");
    }
    if (ctx->world > 1) {                                   // every rank transformed its own rows: the sum is the tensor
        if (hipDeviceSynchronize() != hipSuccess) return fail(TF_ENODEVICE, "AO->MO transformation failed on the device");
        if (ctx->comm) {
            if (comm_allreduce(ctx, *d_out, total, nullptr)) return fail(TF_ENODEVICE, ctx->err);
        } else {
            // the hook sums a buffer whose LAST element is a status word: a rank whose staging failed sends zeros and sets it
            if (hipMemset(*d_out + total, 0, sizeof(double)) != hipSuccess) return fail(TF_ENODEVICE, "AO->MO transformation: memset failed");
            const int arc = ctx->allreduce(ctx->allreduce_user, *d_out, (long long)(total + 1), nullptr);
            if (arc) return fail(TF_ENODEVICE, "AO->MO transformation: the all-reduce hook failed (code " + std::to_string(arc) + ")");
            double status = 0.0;
            if (hipMemcpy(&status, *d_out + total, sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(TF_ENODEVICE, "AO->MO transformation: copy failed");
            if (status != 0.0) return fail(TF_ENODEVICE, "AO->MO transformation: the exchange step failed on a rank: every rank stops");
        }
    }
    if (hipDeviceSynchronize() != hipSuccess) return fail(TF_ENODEVICE, "AO->MO transformation failed on the device");
    if (seconds) *seconds = secs;
    return TF_OK;
}

int tf_ao_to_mo(tf_ctx *ctx, int n1, const double *C1, int n2, const double *C2, int n3, const double *C3, int n4, const double *C4,
                double *out)
{
    if (!ctx) return TF_EINVAL;
    if (!ctx->have_eri) TF_FAIL(ctx, TF_EINVAL, "tf_ao_to_mo: call tf_build_eri first");
    if (n1 < 1 || n2 < 1 || n3 < 1 || n4 < 1 || !C1 || !C2 || !C3 || !C4 || !out) TF_FAIL(ctx, TF_EINVAL, "tf_ao_to_mo: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DeviceBlocks mem;
    double *d_out = nullptr;
    int rc = mo_transform_device(ctx, C1, n1, C2, n2, C3, n3, C4, n4, mem, &d_out, nullptr);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpy(out, d_out, (size_t)n1 * n2 * n3 * n4 * sizeof(double), hipMemcpyDeviceToHost));
    return TF_OK;
}

int tf_mp2_rhf(tf_ctx *ctx, int n_occ, int n_frozen, const double *C, const double *eps, double *e_os, double *e_ss, double *seconds)
{
    int rc = corr_args(ctx, "tf_mp2_rhf", C && eps && e_os && e_ss, "", n_occ, n_frozen);
    if (rc) return rc;
    const int N = ctx->N;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CorrSetup S;
    S.windows(N, n_occ, n_frozen, C);
    const int o = S.o, v = S.v;
    auto t0 = std::chrono::steady_clock::now();
    double e[2];
    {
        DeviceBlocks mem;                                     // (ia|jb), eps and the partials: gone before the clock is read
        double *d_g = nullptr;
        rc = mo_transform_device(ctx, S.Co.data(), o, S.Cv.data(), v, S.Co.data(), o, S.Cv.data(), v, mem, &d_g, nullptr);   // (ia|jb)
        if (rc) return rc;
        double *d_eps = mem.alloc((size_t)N), *d_part = mem.alloc((size_t)2 * CORR_NBLK);
        if (!d_eps || !d_part) TF_FAIL(ctx, TF_ENOMEM, "tf_mp2_rhf: out of device memory");
        HIPCHK(ctx, hipMemcpy(d_eps, eps, (size_t)N * sizeof(double), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(tfmp2::mp2_energy_kernel, dim3(CORR_NBLK), dim3(256), 0, 0, d_g, d_eps, n_frozen, o, v, n_occ, d_part);
        HIPCHK(ctx, sum_partials_host(d_part, CORR_NBLK, 2, e));
    }
    *e_os = e[0]; *e_ss = e[1];
    if (seconds) *seconds = corr_secs(std::chrono::steady_clock::now() - t0);
    return TF_OK;
}

// One UMP2 spin block: sum of tfmp2::ump2_energy_kernel's partials in block order (an empty block is 0 and launches nothing)
static int ump2_block_energy(tf_ctx *ctx, const double *A, const double *B, int o1, int v1, int o2, int v2, const double *eo1, const double *ev1,
                             const double *eo2, const double *ev2, int same_spin, double *d_part, double *sum)
{
    *sum = 0.0;
    if ((long long)o1 * v1 * o2 * v2 == 0) return TF_OK;
    hipLaunchKernelGGL(tfmp2::ump2_energy_kernel, dim3(CORR_NBLK), dim3(256), 0, 0, A, B, o1, v1, o2, v2, eo1, ev1, eo2, ev2, same_spin, d_part);
    double s = 0.0;
    HIPCHK(ctx, sum_partials_host(d_part, CORR_NBLK, 1, &s));
    *sum = s;
    return TF_OK;
}

int tf_mp2_uhf(tf_ctx *ctx, int n_alpha, int n_beta, int n_frozen_alpha, int n_frozen_beta, const double *C_alpha, const double *C_beta,
               const double *eps_alpha, const double *eps_beta, double e_pairs[3], double *seconds)
{
    if (!ctx) return TF_EINVAL;
    if (!ctx->have_eri) TF_FAIL(ctx, TF_EINVAL, "tf_mp2_uhf: call tf_build_eri first");
    const int N = ctx->N;
    if (!C_alpha || !C_beta || !eps_alpha || !eps_beta || !e_pairs || n_frozen_alpha < 0 || n_frozen_alpha > n_alpha || n_frozen_beta < 0 ||
        n_frozen_beta > n_beta || n_alpha >= N || n_beta >= N)
        TF_FAIL(ctx, TF_EINVAL, "tf_mp2_uhf: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const auto t0 = std::chrono::steady_clock::now();
    e_pairs[0] = e_pairs[1] = e_pairs[2] = 0.0;
    if (n_alpha - n_frozen_alpha + n_beta - n_frozen_beta == 0) {   // no correlated electron: every block is empty
        if (seconds) *seconds = corr_secs(std::chrono::steady_clock::now() - t0);
        return TF_OK;
    }
    std::string msg;
    int rc = tfscf::ensure(ctx->scf, N, 6, msg);
    if (rc) { ctx->err = msg; return rc; }
    if (ctx->world > 1 && !ctx->allreduce && !ctx->comm)
        TF_FAIL(ctx, TF_EINVAL, "tf_mp2_uhf on a sharded tensor (world > 1) needs an RCCL communicator (tf_comm_init) or the all-reduce hook (tf_set_allreduce)");
    // host: occupied / virtual windows of both spins, and the stacked bra [C_occ,a | C_occ,b]
    CorrSetup Sa, Sb;
    Sa.windows(N, n_alpha, n_frozen_alpha, C_alpha);
    Sb.windows(N, n_beta, n_frozen_beta, C_beta);
    const int oa = Sa.o, ob = Sb.o, va = Sa.v, vb = Sb.v, n1 = oa + ob;
    const std::vector<double> &Coa = Sa.Co, &Cva = Sa.Cv, &Cob = Sb.Co, &Cvb = Sb.Cv;
    std::vector<double> Cbra((size_t)N * n1);
    for (int m = 0; m < N; ++m) {
        for (int i = 0; i < oa; ++i) Cbra[(size_t)m * n1 + i] = Coa[(size_t)m * oa + i];
        for (int i = 0; i < ob; ++i) Cbra[(size_t)m * n1 + oa + i] = Cob[(size_t)m * ob + i];
    }
    // device eps: occ a | vir a | occ b | vir b, and the energy partials
    DeviceBlocks mem;
    auto fail = [&](int code, const std::string &m) { return corr_fail(ctx, code, m); };
    double *d_eps = mem.alloc((size_t)2 * N), *d_part = d_eps ? mem.alloc((size_t)CORR_NBLK) : nullptr;
    if (!d_eps || !d_part) return fail(TF_ENOMEM, "tf_mp2_uhf: out of device memory");
    if (hipMemcpy(d_eps, eps_alpha + n_frozen_alpha, (size_t)(N - n_frozen_alpha) * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_eps + N, eps_beta + n_frozen_beta, (size_t)(N - n_frozen_beta) * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return fail(TF_ENODEVICE, "tf_mp2_uhf: copy failed");
    const double *eoa = d_eps, *eva = d_eps + oa, *eob = d_eps + N, *evb = d_eps + N + ob;
    double E_ss[2] = {0.0, 0.0}, E_ab = 0.0;
    // the spin-blocked route: packed layout, first quarter on the segments, every occupied space <= 32 and the stacked bra <= 48
    const bool packed = ctx->layout >= 1, tiles = ctx->layout == 2;
    const char *q1env = getenv("TF_MO_Q1");
    const bool spin_blocked = packed && !tiles && !(q1env && q1env[0] == '0') && oa <= 32 && ob <= 32 && n1 <= 48 &&
                              tfmp2::bra1_lds(N, n1) <= ((size_t)150 << 10);
    if (spin_blocked) {
        // L-transforms G_L(aa|aa) | G_L(bb|aa) | G_L(aa|bb) | G_L(bb|bb) | status word of the hook's exchange
        const size_t Baa = (size_t)oa * va * oa * va, Bba = (size_t)ob * vb * oa * va, Bab = (size_t)oa * va * ob * vb, Bbb = (size_t)ob * vb * ob * vb;
        const size_t total = Baa + Bba + Bab + Bbb;
        double *d_G = mem.alloc(total + 1);
        if (!d_G) return fail(TF_ENOMEM, "tf_mp2_uhf: out of device memory");
        double *Gaa = d_G, *Gba = Gaa + Baa, *Gab = Gba + Bba, *Gbb = Gab + Bab;
        double *dCbra = nullptr, *dCoa = nullptr, *dCva = nullptr, *dCob = nullptr, *dCvb = nullptr;
        const size_t nC = (size_t)N * (2 * n1 + va + vb);
        double *d_C = mem.alloc(nC);
        bool ok = d_C != nullptr;
        if (ok) {
            dCbra = d_C; dCoa = dCbra + (size_t)N * n1; dCob = dCoa + (size_t)N * oa; dCva = dCob + (size_t)N * ob; dCvb = dCva + (size_t)N * va;
            const std::vector<double> *hv[5] = {&Cbra, &Coa, &Cob, &Cva, &Cvb};
            double *dv[5] = {dCbra, dCoa, dCob, dCva, dCvb};
            for (int k = 0; k < 5 && ok; ++k) ok = hv[k]->empty() || hipMemcpy(dv[k], hv[k]->data(), hv[k]->size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
            if (!ok) msg = "tf_mp2_uhf: copy failed";
        } else {
            msg = "tf_mp2_uhf: out of device memory";
        }
        if (ok && !grow_mo_pool(ctx, tfmp2::ump2_pool_doubles(N, ctx->n_rows, oa, ob, va, vb) * sizeof(double))) {
            ok = false; msg = "tf_mp2_uhf: out of device memory for the transformation work space";
        }
        int prc = ok ? TF_OK : TF_ENOMEM;
        for (int s = 0; s < 2 && prc == TF_OK; ++s) {          // ket spin a: G_L(aa|aa), G_L(bb|aa); ket spin b: G_L(aa|bb), G_L(bb|bb)
            if ((s ? ob : oa) == 0) continue;
            prc = tfmp2::ump2_spin_pass(ctx->scf.blas, ctx->d_eri(), ctx->d_rowoff, ctx->d_rowsec, ctx->bl, ctx->d_row_ij, ctx->d_rowmap, ctx->n_rows, N,
                                        dCbra, oa, ob, dCva, va, dCvb, vb, s ? dCob : dCoa, s ? ob : oa, s ? dCvb : dCva, s ? vb : va,
                                        s ? Gab : Gaa, s ? Gbb : Gba, ctx->mo_pool(), msg);
        }
        if (ctx->world > 1) {
            // the L-transforms are linear in the rows a rank owns: sum them before the quadratic energy step.  A rank whose part failed
            // sends zeros and a non-zero status word, so that every rank stops together.
            if (hipDeviceSynchronize() != hipSuccess) return fail(TF_ENODEVICE, "tf_mp2_uhf: the transformation failed on the device");
            if (prc != TF_OK && hipMemset(d_G, 0, total * sizeof(double)) != hipSuccess) return fail(TF_ENODEVICE, "tf_mp2_uhf: memset failed");
            const double st = prc != TF_OK ? 1.0 : 0.0;
            if (hipMemcpy(d_G + total, &st, sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return fail(TF_ENODEVICE, "tf_mp2_uhf: copy failed");
            if (ctx->comm) {
                if (comm_allreduce(ctx, d_G, total + 1, nullptr)) return fail(TF_ENODEVICE, ctx->err);
            } else {
                const int arc = ctx->allreduce(ctx->allreduce_user, d_G, (long long)(total + 1), nullptr);
                if (arc) return fail(TF_ENODEVICE, "tf_mp2_uhf: the all-reduce hook failed (code " + std::to_string(arc) + ")");
            }
            double status = 0.0;
            if (hipMemcpy(&status, d_G + total, sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(TF_ENODEVICE, "tf_mp2_uhf: copy failed");
            if (prc != TF_OK) return fail(prc, msg);
            if (status != 0.0) return fail(TF_ENODEVICE, "tf_mp2_uhf: the transformation failed on a rank: every rank stops");
        }
        if (prc != TF_OK) return fail(prc, msg);
        if ((rc = ump2_block_energy(ctx, Gaa, Gaa, oa, va, oa, va, eoa, eva, eoa, eva, 1, d_part, &E_ss[0]))) return rc;
        if ((rc = ump2_block_energy(ctx, Gbb, Gbb, ob, vb, ob, vb, eob, evb, eob, evb, 1, d_part, &E_ss[1]))) return rc;
        if ((rc = ump2_block_energy(ctx, Gab, Gba, oa, va, ob, vb, eoa, eva, eob, evb, 0, d_part, &E_ab))) return rc;
    } else {
        // every other layout, or an occupied space above 32: the general transformation, one complete block (ia|jb) at a time
        struct Blk { const std::vector<double> *Co1, *Cv1, *Co2, *Cv2; int o1, v1, o2, v2; const double *eo1, *ev1, *eo2, *ev2; int same; double *out; };
        const Blk blks[3] = {{&Coa, &Cva, &Coa, &Cva, oa, va, oa, va, eoa, eva, eoa, eva, 1, &E_ss[0]},
                             {&Cob, &Cvb, &Cob, &Cvb, ob, vb, ob, vb, eob, evb, eob, evb, 1, &E_ss[1]},
                             {&Coa, &Cva, &Cob, &Cvb, oa, va, ob, vb, eoa, eva, eob, evb, 0, &E_ab}};
        for (const Blk &k : blks) {
            if ((long long)k.o1 * k.v1 * k.o2 * k.v2 == 0) continue;
            DeviceBlocks blk;
            double *d_g = nullptr;
            if ((rc = mo_transform_device(ctx, k.Co1->data(), k.o1, k.Cv1->data(), k.v1, k.Co2->data(), k.o2, k.Cv2->data(), k.v2, blk, &d_g, nullptr))) return rc;
            if ((rc = ump2_block_energy(ctx, d_g, nullptr, k.o1, k.v1, k.o2, k.v2, k.eo1, k.ev1, k.eo2, k.ev2, k.same, d_part, k.out))) return rc;
        }
    }
    mem.clear();
    e_pairs[0] = 0.5 * E_ss[0];
    e_pairs[1] = 0.5 * E_ss[1];
    e_pairs[2] = E_ab;
    if (seconds) *seconds = corr_secs(std::chrono::steady_clock::now() - t0);
    return TF_OK;
}

// ---- MP3 and what the later methods take from it ----------------------------------------------------------------------------------

// One batch of the AO-direct ladder on the packed layout (null stream): Zh[p][mu][nu] = the stored-triangle contraction of the tensor
// with the pair matrices Tm[p] (tfmp3::mp3_ladder_kernel), p < nb <= TFL_W, everything [N][N] in the internal AO order; Tt [N][N][TFL_W] is
// the work space of the pairs-last image.  The one body behind tf_mp3_rhf and tf_mp3_ladder_probe.  false: a launch failed.
static bool mp3_ladder_batch(tf_ctx *ctx, const double *Tm, int nb, double *Tt, double *Zh)
{
    const int N = ctx->N;
    const long long tot = (long long)N * N * TFL_W;
    int csize[4];
    for (int q = 0; q < 4; ++q) csize[q] = ctx->hl.csize[q];
    hipLaunchKernelGGL(tfmp3::mp3_pairs_last_kernel, dim3((unsigned)std::min<long long>((tot + 255) / 256, 1 << 16)), dim3(256), 0, 0, Tm, N, nb, Tt);
    tfmp3::LadderArgs LA{ctx->d_eri(), ctx->d_rowoff, ctx->d_rowsec, ctx->d_row_ij, ctx->d_rowmap, Tt, Zh, nb, tfmp3::ladder_blocks(csize)};
    tfmp3::launch_ladder(LA, ctx->bl, N, 0);
    return hipGetLastError() == hipSuccess;
}

// dst[a][b][i][j] = (C1_a C2_b|C3_i C4_j), n first-pair and o second-pair orbitals each, dst n n o o doubles on the device: (ab|ij) of
// mp3_mo_blocks and tf_ccsd_rhf's dressed W_ciak block.  In slices of the first index: on the packed and tiles layouts the
// transformation also forms the image with (ab) on the ket side, whose work space grows as N^2 n^2 (190 GB at N = 400); a slice of nc
// orbitals keeps it near 4 GB.  On failure ctx->err is set.
static int mo_vvoo_block(tf_ctx *ctx, const char *who, const std::vector<double> &C1, const std::vector<double> &C2, const std::vector<double> &C3,
                         const std::vector<double> &C4, int o, int v, double *dst)
{
    const int N = ctx->N;
    const long long nn = (long long)N * N;
    const int nc = (int)std::max<long long>(1, std::min<long long>(v, (512LL << 20) / std::max<long long>(1, nn * v)));
    std::vector<double> Cs((size_t)N * nc);
    for (int a0 = 0; a0 < v; a0 += nc) {
        const int na = std::min(nc, v - a0);
        column_window(C1.data(), N, v, a0, na, Cs.data());
        DeviceBlocks slice;
        double *d_s = nullptr;
        const int rc = mo_transform_device(ctx, Cs.data(), na, C2.data(), v, C3.data(), o, C4.data(), o, slice, &d_s, nullptr);
        if (rc) return rc;
        if (hipMemcpy(dst + (size_t)a0 * v * o * o, d_s, (size_t)na * v * o * o * sizeof(double), hipMemcpyDeviceToDevice) != hipSuccess)
            return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": copy failed");
    }
    return TF_OK;
}

// The MO blocks of tf_mp3_rhf and the drivers after it, through mo_transform_device: (ia|jb) = g1[i][a][j][b], (ab|ij) = g2[a][b][i][j],
// (ki|lj) = g3[k][i][l][j], all three mem's.  On failure ctx->err is set.
static int mp3_mo_blocks(tf_ctx *ctx, const char *who, const CorrSetup &S, DeviceBlocks &mem, double **pg1, double **pg2, double **pg3)
{
    const int o = S.o, v = S.v;
    const std::vector<double> &Co = S.Co, &Cv = S.Cv;
    int rc;
    if ((rc = mo_transform_device(ctx, Co.data(), o, Cv.data(), v, Co.data(), o, Cv.data(), v, mem, pg1, nullptr))) return rc;
    if (!(*pg2 = mem.alloc((size_t)v * v * o * o))) return corr_fail(ctx, TF_ENOMEM, std::string(who) + ": out of device memory");
    if ((rc = mo_vvoo_block(ctx, who, Cv, Cv, Co, Co, o, v, *pg2))) return rc;
    return mo_transform_device(ctx, Co.data(), o, Co.data(), o, Co.data(), o, Co.data(), o, mem, pg3, nullptr);
}

// Doubles of the ladder stage's batch work space: U [W][v][N] (later V [W][N][v]) | T [W][N][N] | Tt [N][N][W] (packed) or
// J [chunk][N][N] (exchange route) | Zh [W][N][N]
static size_t mp3_ladder_work_doubles(const tf_ctx *ctx, int v)
{
    const int N = ctx->N, W = TFL_W, chunk = ctx->layout == 2 ? 8 : 2;
    const size_t nn = (size_t)N * N, nU = (size_t)W * v * N, nT = (size_t)W * nn;
    return nU + nT + (ctx->layout == 1 ? nT : (size_t)chunk * nn) + nT;
}

// The particle-particle ladder stage of tf_mp3_rhf and tf_ccd_rhf: Y[ij][a][b] = 1/2 C_v^T Z C_v for the amplitudes too[ij][a][b], in
// batches of TFL_W pairs (packed layout: Z's stored-triangle half through mp3_ladder_batch, the caller adds the transposed pair;
// rows / tiles: the general-density exchange build).  Cvl = C_v in the AO order of T and Z (internal order on the packed layout),
// batch = mp3_ladder_work_doubles of work space.  On failure ctx->err is set.
// With Col (C_o in that AO order; tf_mp4_rhf's singles) every batch is back-transformed with the occupied coefficients as well:
// OA[ij][k][a] = C_o^T Zh_ij C_v and, on the packed layout, OB[ij][a][k] = C_v^T Zh_ij C_o (the other stored-triangle half of
// C_o^T Z_ji C_v); Vo = TFL_W N o doubles of work space.  These GEMMs are skinny and run without rocBLAS's atomics (split-K sums).
// With Bol as well (tf_ccsd_rhf; Bol = C_v t1^T in that AO order, [N][o]) every pair matrix is dressed with c_i b_j^T + b_i c_j^T before the
// contraction (tfccsd::ccsd_dress_pairs_kernel); n_batches, if given, counts the batches.
static int mp3_ladder_stage(tf_ctx *ctx, const char *who, int o, int v, const double *too, const double *Cvl, double *batch, double *Y,
                            const double *Col = nullptr, double *Vo = nullptr, double *OA = nullptr, double *OB = nullptr,
                            const double *Bol = nullptr, long long *n_batches = nullptr)
{
    const int N = ctx->N;
    const long long nn = (long long)N * N;
    const bool packed = ctx->layout == 1;
    rocblas_handle blas = ctx->scf.blas;
    const int W = TFL_W, npair = o * o;
    const size_t nU = (size_t)W * v * N, nT = (size_t)W * nn;
    const int chunk = ctx->layout == 2 ? 8 : 2;
    double *U = batch, *Tm = U + nU, *Tt = Tm + nT, *Jx = Tt, *Zh = Tt + (packed ? nT : (size_t)chunk * nn);
    int rc;
    for (int p0 = 0; p0 < npair; p0 += W) {
        const int nb = std::min(W, npair - p0);
        const double *tb = too + (size_t)p0 * v * v;
        // U_p = t_p C_v^T (packed: Zh of T_p; exchange route: K of T_p^T, so t_p^T), T_p = C_v U_p
        CORR_BLAS(tfmp3::gemm_rm_batched(blas, !packed, true, v, N, v, 1.0, tb, v, (long long)v * v, Cvl, v, 0, 0.0, U, N, (long long)v * N, nb));
        CORR_BLAS(tfmp3::gemm_rm_batched(blas, false, false, N, N, v, 1.0, Cvl, v, 0, U, N, (long long)v * N, 0.0, Tm, N, nn, nb));
        if (Bol) {
            const long long tot = nn * nb;
            hipLaunchKernelGGL(tfccsd::ccsd_dress_pairs_kernel, dim3((unsigned)std::min<long long>((tot + 255) / 256, 1 << 16)), dim3(256), 0, 0, Tm, N, nb,
                               p0, o, Col, Bol, packed ? 0 : 1);
        }
        if (n_batches) ++*n_batches;
        if (packed) {
            if (!mp3_ladder_batch(ctx, Tm, nb, Tt, Zh)) return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": ladder kernel launch failed");
        } else {
            for (int d = 0; d < nb; d += chunk)
                if ((rc = launch_jk_general(ctx, std::min(chunk, nb - d), Tm + (size_t)d * nn, Jx, Zh + (size_t)d * nn))) return rc;
        }
        // V_p = Z_p C_v, Y_p = 1/2 C_v^T V_p
        CORR_BLAS(tfmp3::gemm_rm_batched(blas, false, false, N, v, N, 1.0, Zh, N, nn, Cvl, v, 0, 0.0, U, v, (long long)N * v, nb));
        CORR_BLAS(tfmp3::gemm_rm_batched(blas, true, false, v, v, N, 0.5, Cvl, v, 0, U, v, (long long)N * v, 0.0, Y + (size_t)p0 * v * v, v,
                                         (long long)v * v, nb));
        if (Col) {
            BlasAtomicsOff no_atomics(blas);
            rocblas_status st = tfmp3::gemm_rm_batched(blas, true, false, o, v, N, 1.0, Col, o, 0, U, v, (long long)N * v, 0.0,
                                                       OA + (size_t)p0 * o * v, v, (long long)o * v, nb);
            if (st == rocblas_status_success && packed) {
                st = tfmp3::gemm_rm_batched(blas, false, false, N, o, N, 1.0, Zh, N, nn, Col, o, 0, 0.0, Vo, o, (long long)N * o, nb);
                if (st == rocblas_status_success)
                    st = tfmp3::gemm_rm_batched(blas, true, false, v, o, N, 1.0, Cvl, v, 0, Vo, o, (long long)N * o, 0.0, OB + (size_t)p0 * v * o, o,
                                                (long long)v * o, nb);
            }
            if (st != rocblas_status_success) return corr_fail(ctx, TF_ELINALG, std::string(who) + ": rocBLAS failed in the occupied back-transformation");
        }
    }
    return TF_OK;
}

// The arrays of o^2 v^2 the MP3 stages work on (tf_mp3.hip.h has the expressions), and what they read
struct __attribute__((visibility("hidden"))) Mp3Work {
    double *g1 = nullptr, *g2 = nullptr, *g3 = nullptr;       // the MO blocks of mp3_mo_blocks
    double *tov, *too, *tp, *tsw;                             // the amplitudes in their three layouts, and t' for the energy
    double *M1, *M2, *S13, *S2, *Xhh, *Y, *Moo;               // operands (Moo: o^4) and the terms of X
    double *d_part = nullptr, *d_eps = nullptr;               // partials [3 CORR_NBLK], eps [N]
    double *carve(double *work, long long B2)                 // tov | too | tp | tsw | M1 | M2 | S13 | S2 | Xhh | Y; returns the end
    {
        tov = work; too = tov + B2; tp = too + B2; tsw = tp + B2; M1 = tsw + B2; M2 = M1 + B2; S13 = M2 + B2; S2 = S13 + B2; Xhh = S2 + B2; Y = Xhh + B2;
        return Y + B2;
    }
};

// Stage "amplitudes": t = (ia|jb) / D in the three layouts and the MP2 energies, summed on the host
static int mp3_amplitudes(tf_ctx *ctx, const char *who, const CorrSetup &S, const Mp3Work &W, double e_mp2[2])
{
    hipLaunchKernelGGL(tfmp3::mp3_amp_kernel, dim3(CORR_NBLK), dim3(256), 0, 0, W.g1, W.d_eps, S.n_frozen, S.o, S.v, S.n_occ, W.tov, W.too, W.tp, W.tsw, W.d_part);
    if (sum_partials_host(W.d_part, CORR_NBLK, 2, e_mp2) != hipSuccess) return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": copy failed");
    return TF_OK;
}

// Stage "operands": Moo, M1, M2 from the MO blocks
static void mp3_operands(const CorrSetup &S, const Mp3Work &W)
{
    const long long o4 = (long long)S.o * S.o * S.o * S.o, tot = std::max(S.B2, o4);
    hipLaunchKernelGGL(tfmp3::mp3_operands_kernel, dim3((unsigned)std::min<long long>((tot + 255) / 256, 1 << 16)), dim3(256), 0, 0, W.g1, W.g2, W.g3, S.o, S.v, W.Moo,
                       W.M1, W.M2);
}

// Stage "X[a]": the hole-hole and ring GEMMs on amplitudes a in the three layouts, then mp3_energy_kernel on them and W.Y (the ladder of
// the same amplitudes) and the host sum: e[3].  what names the kernels in the failure message ("MP3", "energy").
static int mp3_hh_ring_energy(tf_ctx *ctx, const char *who, const char *what, const CorrSetup &S, const Mp3Work &W, const double *a_ov,
                              const double *a_oo, const double *a_sw, double e[3])
{
    rocblas_handle blas = ctx->scf.blas;
    const int o = S.o, v = S.v, iov = (int)S.ov, oo = o * o, vv = v * v;
    // Xhh[(ij)][(ab)] = 1/2 Moo[(ij)][(kl)] a[(kl)][(ab)]
    CORR_BLAS(tfmp3::gemm_rm(blas, false, false, oo, vv, oo, 0.5, W.Moo, oo, a_oo, vv, 0.0, W.Xhh, vv));
    // S13 = a_ov M1 - a_sw g1;  S2 = a_sw M2   (all [(ov)][(ov)])
    CORR_BLAS(tfmp3::gemm_rm(blas, false, false, iov, iov, iov, 1.0, a_ov, iov, W.M1, iov, 0.0, W.S13, iov));
    CORR_BLAS(tfmp3::gemm_rm(blas, false, false, iov, iov, iov, -1.0, a_sw, iov, W.g1, iov, 1.0, W.S13, iov));
    CORR_BLAS(tfmp3::gemm_rm(blas, false, false, iov, iov, iov, 1.0, a_sw, iov, W.M2, iov, 0.0, W.S2, iov));
    hipLaunchKernelGGL(tfmp3::mp3_energy_kernel, dim3(CORR_NBLK), dim3(256), 0, 0, W.tp, W.Y, S.packed ? 1 : 0, W.Xhh, W.S13, W.S2, o, v, W.d_part);
    if (sum_partials_host(W.d_part, CORR_NBLK, 3, e) != hipSuccess)
        return corr_fail(ctx, TF_ENODEVICE, std::string(who) + ": the " + what + " kernels failed on the device");
    return TF_OK;
}

// Restricted MP3 (run_restricted_MP3, tuna_mp.py:1410-1470; tf_mp3.hip.h has the expressions).  Stages: the MO blocks (ia|jb),
// (ij|ab), (ki|lj) through mo_transform_device; amplitudes and MP2 partials (mp3_amp_kernel); the particle-particle ladder in the AO
// basis, batches of TFL_W pairs; the hole-hole and ring GEMMs; one energy reduction.
int tf_mp3_rhf(tf_ctx *ctx, int n_occ, int n_frozen, const double *C, const double *eps, double e_mp2[2], double e_mp3[3], double *seconds)
{
    static const char *who = "tf_mp3_rhf";
    int rc = corr_args(ctx, who, C && eps && e_mp2 && e_mp3, " (needs C, eps, outputs and 0 <= n_frozen < n_occ < N)", n_occ, n_frozen);
    if (rc) return rc;
    CorrSetup S;
    if ((rc = corr_begin(ctx, who, n_occ, n_frozen, C, S))) return rc;
    const int o = S.o, v = S.v;
    const long long B2 = S.B2, o4 = (long long)o * o * o * o;
    if (S.ov > 0x7fffffffLL || (long long)v * v > 0x7fffffffLL) TF_FAIL(ctx, TF_EINVAL, "tf_mp3_rhf: dimension overflow");
    DeviceBlocks mem;
    Mp3Work W;
    // ---- MO blocks: (ia|jb) = g1[i][a][j][b], (ab|ij) = g2[a][b][i][j], (ki|lj) = g3[k][i][l][j]
    if ((rc = mp3_mo_blocks(ctx, who, S, mem, &W.g1, &W.g2, &W.g3))) return rc;
    const auto t1 = corr_stamp();
    // ---- work space: tov | too | tp | tsw | M1 | M2 | S13 | S2 | Xhh | Y | Moo
    double *work = mem.alloc((size_t)10 * B2 + (size_t)o4);
    W.d_part = work ? mem.alloc((size_t)3 * CORR_NBLK) : nullptr;
    if (!W.d_part) return corr_fail(ctx, TF_ENOMEM, "tf_mp3_rhf: out of device memory");
    W.Moo = W.carve(work, B2);
    if ((rc = corr_upload(ctx, who, S, mem, eps, nullptr, false, "tf_mp3_rhf: out of device memory"))) return rc;
    W.d_eps = S.d_eps;
    // ---- amplitudes and the MP2 partials
    if ((rc = mp3_amplitudes(ctx, who, S, W, e_mp2))) return rc;
    const auto t2 = corr_stamp();
    // ---- particle-particle ladder: Y[ij][a][b] = 1/2 C_v^T Z C_v, in batches of TFL_W pairs
    double *batch = mem.alloc(mp3_ladder_work_doubles(ctx, v));
    if (!batch) return corr_fail(ctx, TF_ENOMEM, "tf_mp3_rhf: out of device memory for the ladder work space");
    corr_permute(ctx, S);
    if ((rc = mp3_ladder_stage(ctx, who, o, v, W.too, S.Cvl, batch, W.Y))) return rc;
    const auto t3 = corr_stamp();
    // ---- hole-hole and ring terms
    mp3_operands(S, W);
    if ((rc = mp3_hh_ring_energy(ctx, who, "MP3", S, W, W.tov, W.too, W.tsw, e_mp3))) return rc;
    const auto t4 = corr_stamp();
    if (seconds) {
        seconds[0] = corr_secs(t4 - S.t0);
        seconds[1] = corr_secs(t1 - S.t0);
        seconds[2] = corr_secs(t3 - t2);
        seconds[3] = corr_secs((t2 - t1) + (t4 - t3));
    }
    return TF_OK;
}

// Restricted MP4(SDQ) / MP4(DQ) (run_restricted_MP4, tuna_mp.py:1552-1685, without the triples; tf_mp4.hip.h has the expressions).
// Stages: tf_mp3_rhf's own, through its stage functions (so e_mp2 and e_mp3 are bit for bit its values), the first ladder pass also
// back-transforming with C_o for the singles; the singles from those o^3 v values and the block (ki|ld); t2 and a second pass of the
// ladder, hole-hole and ring stages on it; the quadruples' GEMMs.
int tf_mp4_rhf(tf_ctx *ctx, int level, int n_occ, int n_frozen, const double *C, const double *eps, double e_mp2[2], double e_mp3[3], double e_mp4[3],
               double *seconds)
{
    static const char *who = "tf_mp4_rhf";
    int rc = corr_args(ctx, who, C && eps && e_mp2 && e_mp3 && e_mp4, " (needs C, eps, outputs and 0 <= n_frozen < n_occ < N)", n_occ, n_frozen);
    if (rc) return rc;
    if (level != 0 && level != 1) TF_FAIL(ctx, TF_EINVAL, "tf_mp4_rhf: level must be 0 (DQ) or 1 (SDQ)");
    CorrSetup S;
    if ((rc = corr_begin(ctx, who, n_occ, n_frozen, C, S))) return rc;
    const int N = S.N, o = S.o, v = S.v;
    const long long ov = S.ov, B2 = S.B2, o4 = (long long)o * o * o * o, o3v = (long long)o * o * ov;
    if (ov > 0x7fffffffLL || (long long)v * v > 0x7fffffffLL || (long long)o * v * v > 0x7fffffffLL) TF_FAIL(ctx, TF_EINVAL, "tf_mp4_rhf: dimension overflow");
    const bool packed = S.packed, singles = level == 1;
    DeviceBlocks mem;
    Mp3Work W;
    double *g4 = nullptr;
    auto fail = [&](int code, const std::string &m) { return corr_fail(ctx, code, m); };
    // ---- MO blocks: tf_mp3_rhf's, and for the singles (ki|ld) = g4[k][i][l][d]
    if ((rc = mp3_mo_blocks(ctx, who, S, mem, &W.g1, &W.g2, &W.g3))) return rc;
    if (singles && (rc = mo_transform_device(ctx, S.Co.data(), o, S.Co.data(), o, S.Co.data(), o, S.Cv.data(), v, mem, &g4, nullptr))) return rc;
    const auto t1 = corr_stamp();
    // ---- work space: tf_mp3_rhf's tov | too | tp | tsw | M1 | M2 | S13 | S2 | Xhh | Y, then t2's tov2 | too2 | tsw2, then Moo | Ioo (o^4);
    //      small: partials [3 nblk] | sums [4] | eps [N] | F [o^2] | Fv [v^2] | t1 [ov] | singles' partials [ov] | OA [o^3 v] | OB [o^3 v] |
    //      Vo [TFL_W N o]
    const int nblk = CORR_NBLK;
    const size_t nwork = (size_t)13 * B2 + 2 * (size_t)o4;
    const size_t nsmall = (size_t)3 * nblk + 4 + (size_t)N + (size_t)o * o + (size_t)v * v + 2 * (size_t)ov + 2 * (size_t)o3v + (size_t)TFL_W * N * o;
    const size_t nladder = mp3_ladder_work_doubles(ctx, v);
    char oom[160];
    snprintf(oom, sizeof oom, "tf_mp4_rhf: out of device memory for %.2f GB of work space (13 arrays of o^2 v^2 values and the ladder's batch)",
             (double)(nwork + nsmall + nladder) * sizeof(double) / 1e9);
    double *work = mem.alloc(nwork), *d_small = work ? mem.alloc(nsmall) : nullptr, *batch = d_small ? mem.alloc(nladder) : nullptr;
    if (!batch) return fail(TF_ENOMEM, oom);
    double *tov2 = W.carve(work, B2), *too2 = tov2 + B2, *tsw2 = too2 + B2, *Ioo;
    W.Moo = tsw2 + B2; Ioo = W.Moo + o4;
    double *d_part = d_small, *d_sum = d_part + (size_t)3 * nblk, *d_eps = d_sum + 4, *Fjk = d_eps + N, *Fv = Fjk + (size_t)o * o, *d_t1 = Fv + (size_t)v * v,
           *d_spart = d_t1 + ov, *OA = d_spart + ov, *OB = OA + o3v, *Vo = OB + o3v;
    W.d_part = d_part; W.d_eps = d_eps;
    if ((rc = corr_upload(ctx, who, S, mem, eps, d_eps, true, oom))) return rc;
    double *tov = W.tov, *too = W.too, *tp = W.tp, *tsw = W.tsw, *g1 = W.g1;
    // ---- amplitudes and the MP2 partials
    if ((rc = mp3_amplitudes(ctx, who, S, W, e_mp2))) return rc;
    const auto t2 = corr_stamp();
    // ---- first ladder pass, on t: Y and (singles) the occupied-virtual blocks OA, OB
    rocblas_handle blas = ctx->scf.blas;
    corr_permute(ctx, S);
    if ((rc = mp3_ladder_stage(ctx, who, o, v, too, S.Cvl, batch, W.Y, singles ? S.Col : nullptr, Vo, OA, OB))) return rc;
    const auto t3 = corr_stamp();
    const int iov = (int)ov, oo = o * o, vv = v * v, ovv = o * v * v;
    // ---- X[t]: E_MP3
    mp3_operands(S, W);
    if ((rc = mp3_hh_ring_energy(ctx, who, "energy", S, W, tov, too, tsw, e_mp3))) return rc;
    // ---- singles
    e_mp4[0] = 0.0;
    if (singles) {
        hipLaunchKernelGGL(tfmp4::mp4_singles_kernel, dim3((unsigned)ov), dim3(256), 0, 0, too, tp, g4, OA, OB, packed ? 1 : 0, d_eps, n_frozen, n_occ, o, v, d_t1,
                           d_spart);
        hipLaunchKernelGGL(tfccd::cc_sum_partials_kernel, dim3(1), dim3(64), 0, 0, d_spart, (int)ov, 1, d_sum);
        if (hipMemcpy(&e_mp4[0], d_sum, sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(TF_ENODEVICE, "tf_mp4_rhf: the singles kernels failed on the device");
    }
    // ---- t2 = (X[t]_ijab + X[t]_jiba) / D, then X[t2]: E_D
    const dim3 grid_e((unsigned)std::min<long long>((B2 + 255) / 256, 1 << 16));
    hipLaunchKernelGGL(tfmp4::mp4_t2_kernel, grid_e, dim3(256), 0, 0, W.Y, packed ? 1 : 0, W.Xhh, W.S13, W.S2, d_eps, n_frozen, n_occ, o, v, tov2, too2, tsw2);
    const auto t4 = corr_stamp();
    if ((rc = mp3_ladder_stage(ctx, who, o, v, too2, S.Cvl, batch, W.Y))) return rc;
    const auto t5 = corr_stamp();
    double eD[3];
    if ((rc = mp3_hh_ring_energy(ctx, who, "energy", S, W, tov2, too2, tsw2, eD))) return rc;
    e_mp4[1] = eD[0] + eD[1] + eD[2];
    // ---- quadruples, in the buffers the doubles have left: Gx | Gw | Goo | Tmp | QA | QB | QC.  The skinny GEMMs (F, Fv, Ioo) would
    //      otherwise take rocBLAS's split-K kernels, whose sums change from run to run
    double *Gx = W.M1, *Gw = W.M2, *Goo = W.S13, *Tmp = W.S2, *QA = W.Xhh, *QB = W.Y, *QC = tov2;
    BlasAtomicsOff no_atomics(blas);
    hipLaunchKernelGGL(tfmp4::mp4_integral_operands_kernel, grid_e, dim3(256), 0, 0, g1, o, v, Gx, Gw, Goo);
    // QA = 1/2 (t Goo^T) t - F t - t_ij Fv^T
    CORR_BLAS(tfmp3::gemm_rm(blas, false, true, oo, oo, vv, 1.0, too, vv, Goo, vv, 0.0, Ioo, oo));
    CORR_BLAS(tfmp3::gemm_rm(blas, false, false, oo, vv, oo, 0.5, Ioo, oo, too, vv, 0.0, QA, vv));
    CORR_BLAS(tfmp3::gemm_rm(blas, false, true, o, o, ovv, 1.0, tov, ovv, Gw, ovv, 0.0, Fjk, o));
    CORR_BLAS(tfmp3::gemm_rm(blas, false, false, o, ovv, o, -1.0, Fjk, o, too, ovv, 1.0, QA, ovv));
    for (int k = 0; k < o; ++k)
        CORR_BLAS(tfmp3::gemm_rm(blas, false, true, v, v, iov, 1.0, tov + (size_t)k * v * ov, iov, Gw + (size_t)k * v * ov, iov, k ? 1.0 : 0.0, Fv, v));
    CORR_BLAS(tfmp3::gemm_rm_batched(blas, false, true, v, v, v, -1.0, too, v, (long long)vv, Fv, v, 0, 1.0, QA, v, (long long)vv, oo));
    // QB = Tn ((Tn - Tx) Gw)^T + 1/2 Tx (Tx G)^T
    CORR_BLAS(tfmp3::gemm_rm(blas, false, false, iov, iov, iov, 1.0, tov, iov, Gw, iov, 0.0, Tmp, iov));
    CORR_BLAS(tfmp3::gemm_rm(blas, false, false, iov, iov, iov, -1.0, tsw, iov, Gw, iov, 1.0, Tmp, iov));
    CORR_BLAS(tfmp3::gemm_rm(blas, false, true, iov, iov, iov, 1.0, tov, iov, Tmp, iov, 0.0, QB, iov));
    CORR_BLAS(tfmp3::gemm_rm(blas, false, false, iov, iov, iov, 1.0, tsw, iov, g1, iov, 0.0, Tmp, iov));
    CORR_BLAS(tfmp3::gemm_rm(blas, false, true, iov, iov, iov, 0.5, tsw, iov, Tmp, iov, 1.0, QB, iov));
    // QC = 1/2 Tx (Tx Gx)^T
    CORR_BLAS(tfmp3::gemm_rm(blas, false, false, iov, iov, iov, 1.0, tsw, iov, Gx, iov, 0.0, Tmp, iov));
    CORR_BLAS(tfmp3::gemm_rm(blas, false, true, iov, iov, iov, 0.5, tsw, iov, Tmp, iov, 0.0, QC, iov));
    hipLaunchKernelGGL(tfmp4::mp4_energy_kernel, dim3(nblk), dim3(256), 0, 0, tp, QA, QB, QC, o, v, d_part);
    hipLaunchKernelGGL(tfccd::cc_sum_partials_kernel, dim3(1), dim3(64), 0, 0, d_part, nblk, 1, d_sum);
    if (hipMemcpy(&e_mp4[2], d_sum, sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(TF_ENODEVICE, "tf_mp4_rhf: the quadruples kernels failed on the device");
    if (hipGetLastError() != hipSuccess) return fail(TF_ENODEVICE, "tf_mp4_rhf: a kernel launch failed");
    const auto t6 = corr_stamp();
    if (seconds) {
        seconds[0] = corr_secs(t6 - S.t0);
        seconds[1] = corr_secs(t1 - S.t0);
        seconds[2] = corr_secs((t3 - t2) + (t5 - t4));
        seconds[3] = seconds[0] - seconds[1] - seconds[2];
    }
    return TF_OK;
}

// ---- the coupled-cluster loop: what tf_ccd_rhf and tf_ccsd_rhf share ---------------------------------------------------------------

// The GEMM operands both loops have (tf_ccd.hip.h has their definitions).  Every function below issues its GEMMs in the order of
// tf_ccd.hip.h's expressions; the drivers decide where in the step each group stands.
struct __attribute__((visibility("hidden"))) CcOperands {
    int o, v;
    double *g1, *H, *Moo, *Gx, *Gw, *Goo;                     // from the MO blocks, once (cc_guess)
    double *Tn, *Tx, *Tm;                                     // from the amplitudes, every step
    double *A1, *A2, *S1, *S2, *X, *Woo, *Fik, *Fca;
};

// F_ik = Tn [i][(cld)] Gw [k][(cld)]^T;  F_ca = -sum_k Gw_k [c][(ld)] Tn_k [a][(ld)]^T, Tn of the amplitudes the method puts here
static int cc_fik_fca(tf_ctx *ctx, const char *who, const CcOperands &K, const double *Tn)
{
    rocblas_handle blas = ctx->scf.blas;
    const int o = K.o, v = K.v, iov = o * v, ovv = o * v * v;
    const long long ov = (long long)o * v;
    CORR_BLAS(tfmp3::gemm_rm(blas, false, true, o, o, ovv, 1.0, Tn, ovv, K.Gw, ovv, 0.0, K.Fik, o));
    for (int k = 0; k < o; ++k)
        CORR_BLAS(tfmp3::gemm_rm(blas, false, true, v, v, iov, -1.0, K.Gw + (size_t)k * v * ov, iov, Tn + (size_t)k * v * ov, iov, k ? 1.0 : 0.0, K.Fca, v));
    return TF_OK;
}

// W_ijkl += amp [(ij)][(cd)] Goo [(kl)][(cd)]^T (the caller has copied Moo into Woo)
static int cc_woo(tf_ctx *ctx, const char *who, const CcOperands &K, const double *amp)
{
    const int oo = K.o * K.o, vv = K.v * K.v;
    CORR_BLAS(tfmp3::gemm_rm(ctx->scf.blas, false, true, oo, oo, vv, 1.0, amp, vv, K.Goo, vv, 1.0, K.Woo, oo));
    return TF_OK;
}

// A1 += 1/2 Tn Gw - 1/2 Tx G;  A2 -= 1/2 Tx Gx (the caller has put their leading terms there)
static int cc_a1_a2(tf_ctx *ctx, const char *who, const CcOperands &K)
{
    rocblas_handle blas = ctx->scf.blas;
    const int iov = K.o * K.v;
    CORR_BLAS(tfmp3::gemm_rm(blas, false, false, iov, iov, iov, 0.5, K.Tn, iov, K.Gw, iov, 1.0, K.A1, iov));
    CORR_BLAS(tfmp3::gemm_rm(blas, false, false, iov, iov, iov, -0.5, K.Tx, iov, K.g1, iov, 1.0, K.A1, iov));
    CORR_BLAS(tfmp3::gemm_rm(blas, false, false, iov, iov, iov, -0.5, K.Tx, iov, K.Gx, iov, 1.0, K.A2, iov));
    return TF_OK;
}

// X[(ij)][(ab)] = 1/2 W [(ij)][(kl)] amp [(kl)][(ab)]  (with_F: + F_ca^T t_ij - F_ik t);  S1 = A1 Tm - A2 Tn;  S2 = A2 Tx (all [(ov)][(ov)])
static int cc_x_s1_s2(tf_ctx *ctx, const char *who, const CcOperands &K, const double *W, const double *amp, const double *t, bool with_F)
{
    rocblas_handle blas = ctx->scf.blas;
    const int o = K.o, v = K.v, iov = o * v, oo = o * o, vv = v * v, ovv = o * v * v;
    CORR_BLAS(tfmp3::gemm_rm(blas, false, false, oo, vv, oo, 0.5, W, oo, amp, vv, 0.0, K.X, vv));
    if (with_F) {
        CORR_BLAS(tfmp3::gemm_rm_batched(blas, true, false, v, v, v, 1.0, K.Fca, v, 0, t, v, (long long)vv, 1.0, K.X, v, (long long)vv, oo));
        CORR_BLAS(tfmp3::gemm_rm(blas, false, false, o, ovv, o, -1.0, K.Fik, o, t, ovv, 1.0, K.X, ovv));
    }
    CORR_BLAS(tfmp3::gemm_rm(blas, false, false, iov, iov, iov, 1.0, K.A1, iov, K.Tm, iov, 0.0, K.S1, iov));
    CORR_BLAS(tfmp3::gemm_rm(blas, false, false, iov, iov, iov, -1.0, K.A2, iov, K.Tn, iov, 1.0, K.S1, iov));
    CORR_BLAS(tfmp3::gemm_rm(blas, false, false, iov, iov, iov, 1.0, K.A2, iov, K.Tx, iov, 0.0, K.S2, iov));
    return TF_OK;
}

// The part of a step behind the update kernels, the start of the loop and the end of the call.  len = elements of an amplitude vector (o^2 v^2, or
// o^2 v^2 + o v with t1 behind t2); hist = nslot amplitude vectors, then nslot error vectors.
struct __attribute__((visibility("hidden"))) CcLoop {
    const char *who = nullptr;
    const tf_cc_opts *opts = nullptr;
    long long len = 0;
    double *t = nullptr, *t_new = nullptr, *dt = nullptr, *hist = nullptr;
    double *d_part = nullptr, *d_sum = nullptr, *d_coef = nullptr;   // partials [CORR_NBLK][>= nslot], sums and coefficients [>= nslot]
    int *d_slot = nullptr;
    double *e_corr = nullptr, *table = nullptr;               // of the caller's result
    int32_t *n_iter = nullptr, *converged = nullptr;
    tfccd::DiisHistory diis;
    double E = 0.0;
    int code = TF_ENOTCONV;
    bool done = false;
};

// Before the first step: the integral operands (with_g2e: CCSD's G2e_ca as well), the guess t = (ia|jb) / D and its MP2 energy
// (cc_guess_kernel's sums: bit for bit tf_mp2_rhf's); then (ab|ij), which lives on in H, and (ki|lj) are released
static int cc_guess(tf_ctx *ctx, const CcLoop &L, const CorrSetup &S, DeviceBlocks &mem, const CcOperands &K, double *g2, double *g3, double *G2e,
                    double *e_mp2)
{
    const int o = S.o, v = S.v;
    const long long tot = std::max(S.B2, (long long)o * o * o * o);
    hipLaunchKernelGGL(tfccd::cc_integral_operands_kernel, dim3((unsigned)std::min<long long>((tot + 255) / 256, 1 << 16)), dim3(256), 0, 0, K.g1, g2, g3, o, v,
                       K.H, K.Moo, K.Gx, K.Gw, K.Goo);
    if (G2e) hipLaunchKernelGGL(tfccsd::ccsd_g2e_kernel, dim3((unsigned)((v * v + 255) / 256)), dim3(256), 0, 0, K.H, K.g1, o, v, G2e);
    hipLaunchKernelGGL(tfccd::cc_guess_kernel, dim3(CORR_NBLK), dim3(256), 0, 0, K.g1, S.d_eps, S.n_frozen, o, v, S.n_occ, L.t, L.d_part);
    hipLaunchKernelGGL(tfccd::cc_sum_partials_kernel, dim3(1), dim3(64), 0, 0, L.d_part, CORR_NBLK, 2, L.d_sum);
    double e2[2];
    if (hipMemcpy(e2, L.d_sum, sizeof e2, hipMemcpyDeviceToHost) != hipSuccess)
        return corr_fail(ctx, TF_ENODEVICE, std::string(L.who) + ": the guess kernels failed on the device");
    *e_mp2 = e2[0] + e2[1];
    mem.release(g2);
    mem.release(g3);
    return TF_OK;
}

// n sums of the step's reductions to the host
static int cc_read_sums(tf_ctx *ctx, const CcLoop &L, int n, double *red)
{
    if (hipMemcpy(red, L.d_sum, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return corr_fail(ctx, TF_ENODEVICE, std::string(L.who) + ": the iteration kernels failed on the device");
    return TF_OK;
}

// With the step's energy and the norms of its amplitude changes: dE, the table row, the finiteness and convergence tests (L.done: leave
// the loop), then DIIS -- store (t_new, dt); from step 3 on drop the oldest beyond max_diis and extrapolate -- and damping into t
static int cc_advance(tf_ctx *ctx, CcLoop &L, int step, double E, const double *norms, int n_norms)
{
    const tf_cc_opts *opts = L.opts;
    const long long len = L.len;
    auto fail = [&](const char *m) { return corr_fail(ctx, TF_ENODEVICE, std::string(L.who) + m); };
    const double dE = E - L.E;
    L.E = E;
    *L.e_corr = E; *L.n_iter = step;
    if (L.table) { double *row = L.table + 3 * (size_t)(step - 1); row[0] = step; row[1] = E; row[2] = dE; }
    bool finite = std::isfinite(E), small = std::fabs(dE) < opts->conv_delta_E;
    for (int q = 0; q < n_norms; ++q) { finite = finite && std::isfinite(norms[q]); small = small && norms[q] < opts->conv_amplitudes; }
    L.done = true;
    if (!finite || E > 1000.0) { L.code = TF_ELINALG; return TF_OK; }     // tuna_cc.py:3129
    if (small) { L.code = TF_OK; *L.converged = 1; return TF_OK; }
    if (step == opts->max_iter) return TF_OK;
    L.done = false;
    int n_ex = 0;
    if (L.diis.nslot) {
        tfccd::DiisHistory &D = L.diis;
        const int nslot = D.nslot, s = D.store();
        if (hipMemcpyAsync(L.hist + (size_t)s * len, L.t_new, (size_t)len * sizeof(double), hipMemcpyDeviceToDevice, 0) != hipSuccess ||
            hipMemcpyAsync(L.hist + (size_t)(nslot + s) * len, L.dt, (size_t)len * sizeof(double), hipMemcpyDeviceToDevice, 0) != hipSuccess)
            return fail(": copy failed");
        D.drop_oldest(step);
        const int n = (int)D.order.size();
        if (hipMemcpy(L.d_slot, D.order.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return fail(": copy failed");
        hipLaunchKernelGGL(tfccd::cc_diis_dots_kernel, dim3(CORR_NBLK, (unsigned)n), dim3(256), 0, 0, L.hist + (size_t)nslot * len, len, L.d_slot, n, n - 1, len,
                           L.d_part);
        hipLaunchKernelGGL(tfccd::cc_sum_partials_kernel, dim3(1), dim3(64), 0, 0, L.d_part, CORR_NBLK, n, L.d_sum);
        std::vector<double> row(n), coef(n);
        if (hipMemcpy(row.data(), L.d_sum, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(": the DIIS kernels failed on the device");
        D.enter_dots(s, row.data());
        if (step > 2 && D.solve(coef.data())) {
            if (hipMemcpy(L.d_coef, coef.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return fail(": copy failed");
            n_ex = n;
        }
    }
    hipLaunchKernelGGL(tfccd::cc_mix_kernel, dim3((unsigned)std::min<long long>((len + 255) / 256, 1 << 16)), dim3(256), 0, 0, L.t, L.t_new, L.hist, len, L.d_slot,
                       L.d_coef, n_ex, opts->damping, len);
    return TF_OK;
}

// After the loop and the caller's copies (t_end = its stamp): the seconds and how the loop ended
static int cc_report(tf_ctx *ctx, const CcLoop &L, std::chrono::steady_clock::time_point t0, std::chrono::steady_clock::time_point t_blocks,
                     std::chrono::steady_clock::time_point t_end, double ladder_seconds, double seconds[4])
{
    seconds[0] = corr_secs(t_end - t0);
    seconds[1] = corr_secs(t_blocks - t0);
    seconds[2] = ladder_seconds;
    seconds[3] = seconds[0] - seconds[1] - seconds[2];
    if (L.code == TF_ELINALG) TF_FAIL(ctx, TF_ELINALG, "%s: non-finite amplitudes or energy in step %d (try stronger damping)", L.who, (int)*L.n_iter);
    if (L.code == TF_ENOTCONV) TF_FAIL(ctx, TF_ENOTCONV, "%s: the iterations did not converge in %d steps", L.who, (int)L.opts->max_iter);
    return TF_OK;
}

// Restricted LCCD / CCD (tuna_cc.py:830-864, :915-960, the loop of :3004-3161; tf_ccd.hip.h has the expressions and the operands).
// Stages: the MO blocks of tf_mp3_rhf, once; per step the amplitude operands, the ladder stage of tf_mp3_rhf on the current amplitudes,
// CCD's intermediates, the hole-hole and ring GEMMs, the fused update; then convergence, DIIS and damping (cc_advance).  Only dE, ||dt||
// and the new row of the DIIS matrix come back to the host per step.
int tf_ccd_rhf(tf_ctx *ctx, const tf_cc_opts *opts, int n_occ, int n_frozen, const double *C, const double *eps, tf_cc_result *out)
{
    static const char *who = "tf_ccd_rhf";
    int rc = corr_args(ctx, who, opts && C && eps && out, " (needs opts, C, eps, out and 0 <= n_frozen < n_occ < N)", n_occ, n_frozen);
    if (rc) return rc;
    if (opts->max_iter < 1) TF_FAIL(ctx, TF_EINVAL, "tf_ccd_rhf: max_iter must be at least 1");
    if (opts->method != 0 && opts->method != 1) TF_FAIL(ctx, TF_EINVAL, "tf_ccd_rhf: method must be 0 (LCCD) or 1 (CCD)");
    CorrSetup S;
    if ((rc = corr_begin(ctx, who, n_occ, n_frozen, C, S))) return rc;
    const int N = S.N, o = S.o, v = S.v;
    const long long ov = S.ov, B2 = S.B2, o4 = (long long)o * o * o * o;
    if (ov > 0x7fffffffLL || (long long)o * v * v > 0x7fffffffLL) TF_FAIL(ctx, TF_EINVAL, "tf_ccd_rhf: dimension overflow");
    const bool packed = S.packed, ccd = opts->method == 1;
    CcLoop L;
    L.who = who; L.opts = opts; L.len = B2;
    L.e_corr = &out->e_corr; L.table = out->table; L.n_iter = &out->n_iter; L.converged = &out->converged;
    L.diis.init(opts->use_diis != 0, opts->max_diis);
    const int nslot = L.diis.nslot;
    out->e_corr = out->e_mp2 = 0.0; out->n_iter = 0; out->converged = 0;
    DeviceBlocks mem;
    double *g1 = nullptr, *g2 = nullptr, *g3 = nullptr;
    auto fail = [&](int code, const std::string &m) { return corr_fail(ctx, code, m); };
    // ---- MO blocks, as tf_mp3_rhf makes them
    if ((rc = mp3_mo_blocks(ctx, who, S, mem, &g1, &g2, &g3))) return rc;
    const auto t1 = corr_stamp();
    // ---- work space, in arrays of o^2 v^2: t | t_new | dt | Tn | Tx | Tm | S1 | S2 | X | Y | H  (CCD: | A1 | A2 | Gx | Gw | Goo), then
    //      Moo, W (o^4 each), F_ik, F_ca; the DIIS history: nslot amplitude vectors, then nslot error vectors
    const int nblk = CORR_NBLK;
    const size_t narr = ccd ? 16 : 11;
    const size_t nwork = narr * (size_t)B2 + 2 * (size_t)o4 + (size_t)o * o + (size_t)v * v;
    const size_t nsmall = (size_t)nblk * std::max(2, nslot) + 2 * (size_t)std::max(2, nslot) + (size_t)N;
    const size_t nladder = mp3_ladder_work_doubles(ctx, v);
    char oom[160];
    snprintf(oom, sizeof oom, "tf_ccd_rhf: out of device memory for %.2f GB of work space (%zu arrays of o^2 v^2 values)",
             (double)(nwork + 2 * (size_t)nslot * B2 + nladder) * sizeof(double) / 1e9, narr + 2 * (size_t)nslot);
    double *work = mem.alloc(nwork);
    L.hist = work && nslot ? mem.alloc(2 * (size_t)nslot * B2) : nullptr;
    double *batch = work && (L.hist || !nslot) ? mem.alloc(nladder) : nullptr, *d_small = batch ? mem.alloc(nsmall) : nullptr;
    L.d_slot = d_small ? mem.alloc_int((size_t)std::max(1, nslot)) : nullptr;
    if (!L.d_slot) return fail(TF_ENOMEM, oom);
    double *t = work, *t_new = t + B2, *dt = t_new + B2, *Tn = dt + B2, *Tx = Tn + B2, *Tm = Tx + B2, *S1 = Tm + B2, *S2 = S1 + B2, *X = S2 + B2,
           *Y = X + B2, *H = Y + B2, *A1 = g1, *A2 = H, *Gx = nullptr, *Gw = nullptr, *Goo = nullptr, *tail = H + B2;
    if (ccd) { A1 = tail; A2 = A1 + B2; Gx = A2 + B2; Gw = Gx + B2; Goo = Gw + B2; tail = Goo + B2; }
    double *Moo = tail, *Woo = Moo + o4, *Fik = Woo + o4, *Fca = Fik + (size_t)o * o;
    double *d_part = d_small, *d_sum = d_part + (size_t)nblk * std::max(2, nslot), *d_coef = d_sum + std::max(2, nslot), *d_eps = d_coef + std::max(2, nslot);
    L.t = t; L.t_new = t_new; L.dt = dt; L.d_part = d_part; L.d_sum = d_sum; L.d_coef = d_coef;
    if ((rc = corr_upload(ctx, who, S, mem, eps, d_eps, false, oom))) return rc;
    corr_permute(ctx, S);
    const dim3 grid_e((unsigned)std::min<long long>((B2 + 255) / 256, 1 << 16));
    // ---- the integral operands, the guess amplitudes and their MP2 energy
    const CcOperands K{o, v, g1, H, Moo, Gx, Gw, Goo, Tn, Tx, Tm, A1, A2, S1, S2, X, Woo, Fik, Fca};
    if ((rc = cc_guess(ctx, L, S, mem, K, g2, g3, nullptr, &out->e_mp2))) return rc;
    // the iteration's GEMMs run without atomics (the skinny ones -- F_ik, W_ijkl -- would otherwise take rocBLAS's split-K kernels, whose
    // sums change from run to run); the AO->MO transformation above keeps them, as everywhere else
    BlasAtomicsOff no_atomics(ctx->scf.blas);
    double ladder_seconds = 0.0;
    for (int step = 1; step <= opts->max_iter; ++step) {
        hipLaunchKernelGGL(tfccd::cc_amplitude_operands_kernel, grid_e, dim3(256), 0, 0, t, o, v, Tn, Tx, Tm);
        // ---- particle-particle ladder on the bare (ac|bd): Y[ij][a][b]
        const auto l0 = corr_stamp();
        if ((rc = mp3_ladder_stage(ctx, who, o, v, t, S.Cvl, batch, Y))) return rc;
        const auto l1 = corr_stamp();
        ladder_seconds += corr_secs(l1 - l0);
        const double *W = Moo;
        if (ccd) {
            if ((rc = cc_fik_fca(ctx, who, K, Tn))) return rc;
            // W_ijkl = Moo + t Goo^T;  A1 = G + ...;  A2 = H - ...
            if (hipMemcpyAsync(Woo, Moo, (size_t)o4 * sizeof(double), hipMemcpyDeviceToDevice, 0) != hipSuccess ||
                hipMemcpyAsync(A1, g1, (size_t)B2 * sizeof(double), hipMemcpyDeviceToDevice, 0) != hipSuccess ||
                hipMemcpyAsync(A2, H, (size_t)B2 * sizeof(double), hipMemcpyDeviceToDevice, 0) != hipSuccess)
                return fail(TF_ENODEVICE, "tf_ccd_rhf: copy failed");
            if ((rc = cc_woo(ctx, who, K, t))) return rc;
            W = Woo;
            if ((rc = cc_a1_a2(ctx, who, K))) return rc;
        }
        if ((rc = cc_x_s1_s2(ctx, who, K, W, t, t, ccd))) return rc;
        // ---- the fused update: t_new, dt, E and ||dt||^2
        hipLaunchKernelGGL(tfccd::cc_update_kernel, dim3(nblk), dim3(256), 0, 0, g1, d_eps, n_frozen, n_occ, o, v, t, Y, packed ? 1 : 0, X, S1, S2, t_new, dt,
                           d_part);
        hipLaunchKernelGGL(tfccd::cc_sum_partials_kernel, dim3(1), dim3(64), 0, 0, d_part, nblk, 2, d_sum);
        double red[2];
        if ((rc = cc_read_sums(ctx, L, 2, red))) return rc;
        const double dnorm = std::sqrt(red[1]);
        if ((rc = cc_advance(ctx, L, step, red[0], &dnorm, 1))) return rc;
        if (L.done) break;
    }
    if (hipGetLastError() != hipSuccess) return fail(TF_ENODEVICE, "tf_ccd_rhf: a kernel launch failed");
    if (out->t2 && hipMemcpy(out->t2, t_new, (size_t)B2 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(TF_ENODEVICE, "tf_ccd_rhf: copy failed");
    const auto t4 = corr_stamp();
    return cc_report(ctx, L, S.t0, t1, t4, ladder_seconds, out->seconds);
}

// Restricted LCCSD / QCISD / CCSD (tuna_cc.py:1020-1063, :1503-1557, :1638-1718, the loop of :3004-3161; tf_ccsd.hip.h has the expressions).
// tf_ccd_rhf's stages with t1 directly behind t2 in every amplitude buffer (o^2 v^2 + o v elements): per step the amplitude operands, ONE
// ladder pass on the dressed pair matrices with the occupied back-transformation of tf_mp4_rhf, the intermediates (CCSD: two dressed
// AO->MO transformations and one general-density J/K build), the GEMMs, the fused singles and doubles updates; then convergence, DIIS and
// damping over both blocks.  Work space in arrays of o^2 v^2: t | t_new | dt (each o v longer) | Tn | Tx | Tm | S1 | S2 | X | Y | H
// (QCISD, CCSD: | A1 | A2 | Gx | Gw | Goo) (CCSD: | th | Q) -- 11, 16, 18 -- then Moo, W (o^4), F_ik, F_ca, G2e, F_kc, OA, OB (o^3 v), the
// stage's Vo, C_v t1^T and an N max(o, v) scratch; nothing with three or four virtual indices.
int tf_ccsd_rhf(tf_ctx *ctx, const tf_cc_opts *opts, int n_occ, int n_frozen, const double *C, const double *eps, tf_ccsd_result *out)
{
    static const char *who = "tf_ccsd_rhf";
    int rc = corr_args(ctx, who, opts && C && eps && out, " (needs opts, C, eps, out and 0 <= n_frozen < n_occ < N)", n_occ, n_frozen);
    if (rc) return rc;
    if (opts->max_iter < 1) TF_FAIL(ctx, TF_EINVAL, "tf_ccsd_rhf: max_iter must be at least 1");
    if (opts->method != TF_CCSD_LCCSD && opts->method != TF_CCSD_QCISD && opts->method != TF_CCSD_CCSD)
        TF_FAIL(ctx, TF_EINVAL, "tf_ccsd_rhf: method must be 0 (LCCSD), 1 (QCISD) or 2 (CCSD)");
    CorrSetup S;
    if ((rc = corr_begin(ctx, who, n_occ, n_frozen, C, S))) return rc;
    const int N = S.N, o = S.o, v = S.v;
    const long long ov = S.ov, B2 = S.B2, BT = B2 + ov, o4 = (long long)o * o * o * o, o3v = (long long)o * o * ov, nn = (long long)N * N;
    if (ov > 0x7fffffffLL || (long long)o * v * v > 0x7fffffffLL || o4 > 0x7fffffffLL) TF_FAIL(ctx, TF_EINVAL, "tf_ccsd_rhf: dimension overflow");
    const int level = opts->method;
    const bool packed = S.packed, quad = level >= 1, full = level >= 2;
    const std::vector<double> &Co = S.Co, &Cv = S.Cv;
    CcLoop L;
    L.who = who; L.opts = opts; L.len = BT;
    L.e_corr = &out->e_corr; L.table = out->table; L.n_iter = &out->n_iter; L.converged = &out->converged;
    L.diis.init(opts->use_diis != 0, opts->max_diis);
    const int nslot = L.diis.nslot;
    out->e_corr = out->e_mp2 = out->e_singles = out->e_connected = out->e_disconnected = out->t1_norm = 0.0;
    out->n_iter = 0; out->converged = 0; out->ladder_batches = 0;
    DeviceBlocks mem;
    double *g1 = nullptr, *g2 = nullptr, *g3 = nullptr, *g4 = nullptr;
    auto fail = [&](int code, const std::string &m) { return corr_fail(ctx, code, m); };
    // ---- MO blocks: tf_mp3_rhf's, and (ik|ja) = g4[i][k][j][a]
    if ((rc = mp3_mo_blocks(ctx, who, S, mem, &g1, &g2, &g3))) return rc;
    if ((rc = mo_transform_device(ctx, Co.data(), o, Co.data(), o, Co.data(), o, Cv.data(), v, mem, &g4, nullptr))) return rc;
    const auto t1s = corr_stamp();
    const int nblk = CORR_NBLK;
    const size_t narr = full ? 18 : (quad ? 16 : 11);
    const int ntmp = std::max(o, v);
    const size_t nwork = narr * (size_t)B2 + 3 * (size_t)ov + 2 * (size_t)o4 + (size_t)o * o + 2 * (size_t)v * v + (size_t)ov + 2 * (size_t)o3v +
                         (size_t)TFL_W * N * o + (size_t)N * o + (size_t)N * ntmp;
    const int nsum = std::max(4, nslot), npart = std::max(2, nslot);
    const size_t nsmall = (size_t)nblk * npart + (size_t)nblk + (size_t)ov + (size_t)nsum + (size_t)npart + (size_t)N;
    const size_t nladder = mp3_ladder_work_doubles(ctx, v);
    char oom[160];
    snprintf(oom, sizeof oom, "tf_ccsd_rhf: out of device memory for %.2f GB of work space (%zu arrays of o^2 v^2 values)",
             (double)(nwork + 2 * (size_t)nslot * BT + nladder) * sizeof(double) / 1e9, narr + 2 * (size_t)nslot);
    double *work = mem.alloc(nwork);
    L.hist = work && nslot ? mem.alloc(2 * (size_t)nslot * BT) : nullptr;
    double *batch = work && (L.hist || !nslot) ? mem.alloc(nladder) : nullptr, *d_small = batch ? mem.alloc(nsmall) : nullptr;
    L.d_slot = d_small ? mem.alloc_int((size_t)std::max(1, nslot)) : nullptr;
    if (!L.d_slot) return fail(TF_ENOMEM, oom);
    double *t = work, *t_new = t + BT, *dt = t_new + BT, *Tn = dt + BT, *Tx = Tn + B2, *Tm = Tx + B2, *S1 = Tm + B2, *S2 = S1 + B2, *X = S2 + B2,
           *Y = X + B2, *H = Y + B2, *A1 = g1, *A2 = H, *Gx = nullptr, *Gw = nullptr, *Goo = nullptr, *th = t, *Q = nullptr, *tail = H + B2;
    if (quad) { A1 = tail; A2 = A1 + B2; Gx = A2 + B2; Gw = Gx + B2; Goo = Gw + B2; tail = Goo + B2; }
    if (full) { th = tail; Q = th + B2; tail = Q + B2; }
    double *Moo = tail, *Woo = Moo + o4, *Fik = Woo + o4, *Fca = Fik + (size_t)o * o, *G2e = Fca + (size_t)v * v, *Fkc = G2e + (size_t)v * v,
           *OA = Fkc + ov, *OB = OA + o3v, *Vo = OB + o3v, *Bol = Vo + (size_t)TFL_W * N * o, *d_tmp = Bol + (size_t)N * o;
    double *d_part = d_small, *d_part2 = d_part + (size_t)nblk * npart, *d_spart = d_part2 + nblk, *d_sum = d_spart + ov, *d_coef = d_sum + nsum,
           *d_eps = d_coef + npart;
    double *t1 = t + B2, *t1_new = t_new + B2, *dt1 = dt + B2;
    L.t = t; L.t_new = t_new; L.dt = dt; L.d_part = d_part; L.d_sum = d_sum; L.d_coef = d_coef;
    if ((rc = corr_upload(ctx, who, S, mem, eps, d_eps, true, oom))) return rc;
    if (hipMemset(t1, 0, (size_t)ov * sizeof(double)) != hipSuccess) return fail(TF_ENODEVICE, "tf_ccsd_rhf: copy failed");
    corr_permute(ctx, S);
    const double *Cvl = S.Cvl, *Col = S.Col, *d_Cv = S.d_Cv, *d_Co = S.d_Co;
    const dim3 grid_e((unsigned)std::min<long long>((B2 + 255) / 256, 1 << 16));
    // ---- the integral operands, the guess amplitudes and their MP2 energy
    const CcOperands K{o, v, g1, H, Moo, Gx, Gw, Goo, Tn, Tx, Tm, A1, A2, S1, S2, X, Woo, Fik, Fca};
    if ((rc = cc_guess(ctx, L, S, mem, K, g2, g3, G2e, &out->e_mp2))) return rc;
    rocblas_handle blas = ctx->scf.blas;
    BlasAtomicsOff no_atomics(blas);
    const int iov = (int)ov;
    std::vector<double> h_t1((size_t)ov), Lo, Xv, Bh, Ph;
    if (full) { Lo.resize((size_t)N * o); Xv.resize((size_t)N * v); Bh.resize((size_t)N * o); Ph.resize((size_t)nn); }
    double ladder_seconds = 0.0;
    long long batches = 0;
    for (int step = 1; step <= opts->max_iter; ++step) {
        hipLaunchKernelGGL(tfccd::cc_amplitude_operands_kernel, grid_e, dim3(256), 0, 0, t, o, v, Tn, Tx, Tm);
        if (full) hipLaunchKernelGGL(tfccsd::ccsd_tau_kernel, grid_e, dim3(256), 0, 0, t, t1, o, v, th);
        // ---- the one ladder pass of the step, on the dressed pair matrices: Y, OA, OB
        CORR_BLAS(tfmp3::gemm_rm(blas, false, true, N, o, v, 1.0, Cvl, v, t1, v, 0.0, Bol, o));
        const auto l0 = corr_stamp();
        if ((rc = mp3_ladder_stage(ctx, who, o, v, th, Cvl, batch, Y, Col, Vo, OA, OB, Bol, &batches))) return rc;
        const auto l1 = corr_stamp();
        ladder_seconds += corr_secs(l1 - l0);
        const double *W = Moo;
        if (quad) {
            // F_ik, F_ca as tf_ccd_rhf's, on th (CCSD: its operand goes through S1, free until the ring GEMMs)
            const double *Tnh = Tn;
            if (full) {
                hipLaunchKernelGGL(tfccd::cc_amplitude_operands_kernel, grid_e, dim3(256), 0, 0, th, o, v, S1, S2, X);
                Tnh = S1;
            }
            if ((rc = cc_fik_fca(ctx, who, K, Tnh))) return rc;
            hipLaunchKernelGGL(tfccsd::ccsd_fkc_kernel, dim3((unsigned)ov), dim3(256), 0, 0, Gw, t1, iov, Fkc);
        }
        // ---- the fused singles update, on F_ik and F_ca as they stand (CCSD dresses them to L_ik, L_ca for the doubles below)
        hipLaunchKernelGGL(tfccsd::ccsd_singles_kernel, dim3((unsigned)ov), dim3(256), 0, 0, level, t, th, t1, g4, OA, OB, packed ? 1 : 0, G2e, Fik, Fca, Fkc, d_eps,
                           n_frozen, n_occ, o, v, t1_new, dt1, d_spart);
        if (quad) {
            if (hipMemcpyAsync(Woo, Moo, (size_t)o4 * sizeof(double), hipMemcpyDeviceToDevice, 0) != hipSuccess) return fail(TF_ENODEVICE, "tf_ccsd_rhf: copy failed");
            if ((rc = cc_woo(ctx, who, K, th))) return rc;
            W = Woo;
            if (!full) {
                if (hipMemcpyAsync(A1, g1, (size_t)B2 * sizeof(double), hipMemcpyDeviceToDevice, 0) != hipSuccess ||
                    hipMemcpyAsync(A2, H, (size_t)B2 * sizeof(double), hipMemcpyDeviceToDevice, 0) != hipSuccess)
                    return fail(TF_ENODEVICE, "tf_ccsd_rhf: copy failed");
            } else {
                hipLaunchKernelGGL(tfccsd::ccsd_woo_dress_kernel, dim3((unsigned)((o4 + 255) / 256)), dim3(256), 0, 0, g4, t1, o, v, Woo);
                // the dressed coefficients L = C_o + C_v t1^T, X = C_v - C_o t1 and the density C_v t1^T C_o^T, on the host (N o v flops)
                if (hipMemcpy(h_t1.data(), t1, (size_t)ov * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(TF_ENODEVICE, "tf_ccsd_rhf: copy failed");
                for (int m = 0; m < N; ++m) {
                    for (int i = 0; i < o; ++i) {
                        double b = 0.0;
                        for (int a = 0; a < v; ++a) b += Cv[(size_t)m * v + a] * h_t1[(size_t)i * v + a];
                        Bh[(size_t)m * o + i] = b;
                        Lo[(size_t)m * o + i] = Co[(size_t)m * o + i] + b;
                    }
                    for (int a = 0; a < v; ++a) {
                        double x = 0.0;
                        for (int k = 0; k < o; ++k) x += Co[(size_t)m * o + k] * h_t1[(size_t)k * v + a];
                        Xv[(size_t)m * v + a] = Cv[(size_t)m * v + a] - x;
                    }
                }
                for (int m = 0; m < N; ++m)
                    for (int n = 0; n < N; ++n) {
                        double p = 0.0;
                        for (int k = 0; k < o; ++k) p += Bh[(size_t)m * o + k] * Co[(size_t)n * o + k];
                        Ph[(size_t)m * N + n] = p;
                    }
                // W_icak's t1 part (l_i x_a|kc) -> A1, W_ciak's (l_i k|x_a c) -> A2
                {
                    DeviceBlocks dressed;
                    double *d_a = nullptr;
                    if ((rc = mo_transform_device(ctx, Lo.data(), o, Xv.data(), v, Co.data(), o, Cv.data(), v, dressed, &d_a, nullptr))) return rc;
                    if (hipMemcpy(A1, d_a, (size_t)B2 * sizeof(double), hipMemcpyDeviceToDevice) != hipSuccess) return fail(TF_ENODEVICE, "tf_ccsd_rhf: copy failed");
                }
                if ((rc = mo_vvoo_block(ctx, who, Xv, Cv, Lo, Co, o, v, Q))) return rc;
                hipLaunchKernelGGL(tfccsd::ccsd_vvoo_operand_kernel, grid_e, dim3(256), 0, 0, Q, o, v, A2);
                // M = 2 J - K of that density; L_ca = F_ca + C_v^T M C_v, L_ik = F_ik + C_o^T M C_o
                if (hipMemcpy(ctx->jk.all.P, Ph.data(), (size_t)nn * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return fail(TF_ENODEVICE, "tf_ccsd_rhf: copy failed");
                if ((rc = launch_jk_general(ctx, 1, ctx->jk.all.P, ctx->jk.all.J, ctx->jk.all.K))) return rc;
                hipLaunchKernelGGL(tfccsd::ccsd_m_kernel, dim3((unsigned)std::min<long long>((nn + 255) / 256, 1 << 16)), dim3(256), 0, 0, ctx->jk.all.J, ctx->jk.all.K, nn);
                CORR_BLAS(tfmp3::gemm_rm(blas, false, false, N, v, N, 1.0, ctx->jk.all.J, N, d_Cv, v, 0.0, d_tmp, v));
                CORR_BLAS(tfmp3::gemm_rm(blas, true, false, v, v, N, 1.0, d_Cv, v, d_tmp, v, 1.0, Fca, v));
                CORR_BLAS(tfmp3::gemm_rm(blas, false, false, N, o, N, 1.0, ctx->jk.all.J, N, d_Co, o, 0.0, d_tmp, o));
                CORR_BLAS(tfmp3::gemm_rm(blas, true, false, o, o, N, 1.0, d_Co, o, d_tmp, o, 1.0, Fik, o));
            }
            if ((rc = cc_a1_a2(ctx, who, K))) return rc;
        }
        if ((rc = cc_x_s1_s2(ctx, who, K, W, th, t, quad))) return rc;
        // ---- the fused doubles update, then the disconnected energy of the new singles
        hipLaunchKernelGGL(tfccsd::ccsd_update_kernel, dim3(nblk), dim3(256), 0, 0, level, g1, d_eps, n_frozen, n_occ, o, v, t, Y, packed ? 1 : 0, X, S1, S2, g4, t1,
                           OA, OB, t_new, dt, d_part);
        hipLaunchKernelGGL(tfccd::cc_sum_partials_kernel, dim3(1), dim3(64), 0, 0, d_part, nblk, 2, d_sum);
        hipLaunchKernelGGL(tfccd::cc_sum_partials_kernel, dim3(1), dim3(64), 0, 0, d_spart, (int)ov, 1, d_sum + 2);
        if (full) {
            hipLaunchKernelGGL(tfccsd::ccsd_disconnected_kernel, dim3(nblk), dim3(256), 0, 0, g1, t1_new, o, v, d_part2);
            hipLaunchKernelGGL(tfccd::cc_sum_partials_kernel, dim3(1), dim3(64), 0, 0, d_part2, nblk, 1, d_sum + 3);
        }
        double red[4] = {0.0, 0.0, 0.0, 0.0};
        if ((rc = cc_read_sums(ctx, L, full ? 4 : 3, red))) return rc;
        out->e_connected = red[0];
        out->e_disconnected = full ? red[3] : 0.0;
        const double norms[2] = {std::sqrt(red[1]), std::sqrt(red[2])};
        if ((rc = cc_advance(ctx, L, step, out->e_singles + out->e_connected + out->e_disconnected, norms, 2))) return rc;
        if (L.done) break;
    }
    if (hipGetLastError() != hipSuccess) return fail(TF_ENODEVICE, "tf_ccsd_rhf: a kernel launch failed");
    if (hipMemcpy(h_t1.data(), t1_new, (size_t)ov * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        (out->t2 && hipMemcpy(out->t2, t_new, (size_t)B2 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess))
        return fail(TF_ENODEVICE, "tf_ccsd_rhf: copy failed");
    {
        double s = 0.0;
        for (long long e = 0; e < ov; ++e) s += h_t1[(size_t)e] * h_t1[(size_t)e];
        out->t1_norm = std::sqrt(s);
        if (out->t1) std::memcpy(out->t1, h_t1.data(), (size_t)ov * sizeof(double));
    }
    out->ladder_batches = batches;
    const auto t4 = corr_stamp();
    return cc_report(ctx, L, S.t0, t1s, t4, ladder_seconds, out->seconds);
}

// The perturbative triples of CCSD(T), QCISD(T) and full MP4 (tuna_cc.py:2688-2758, tuna_mp.py:403-428 and :1605-1637; tf_triples.hip.h has
// the expressions and the fused kernel).  Stages: the blocks (ia|jb) and (ki|ld) as tf_ccsd_rhf makes them; (ia|bc) = [i][a][b][c], resident,
// filled in slabs of occupied orbitals (TF_TRIPLES_SLAB bounds them) and slices of b (TF_TRIPLES_SLICE), both sized from the free memory: the transformation
// holds N^2 values per element of its ket pair; then per unordered triple i >= j >= k (i = j = k skipped) twelve rocBLAS GEMMs write the
// six X_pqr, one launch of triples_energy_kernel and one of triples_sum_partials_kernel leave two sums per triple on the device.  The host
// reads them once after the loop and adds them in loop order with the number of distinct orderings of each triple.
int tf_triples_rhf(tf_ctx *ctx, int kind, int n_occ, int n_frozen, const double *C, const double *eps, const double *t1, const double *t2,
                   tf_triples_result *out)
{
    static const char *who = "tf_triples_rhf";
    int rc = corr_args(ctx, who, C && eps && out, " (needs C, eps, out and 0 <= n_frozen < n_occ < N)", n_occ, n_frozen);
    if (rc) return rc;
    if (kind != TF_TRIPLES_CCSD_T && kind != TF_TRIPLES_QCISD_T && kind != TF_TRIPLES_MP4)
        TF_FAIL(ctx, TF_EINVAL, "tf_triples_rhf: kind must be 0 (CCSD(T)), 1 (QCISD(T)) or 2 (MP4)");
    CorrSetup S;
    if ((rc = corr_begin(ctx, who, n_occ, n_frozen, C, S))) return rc;
    if (kind == TF_TRIPLES_MP4 && (t1 || t2)) TF_FAIL(ctx, TF_EINVAL, "tf_triples_rhf: MP4 makes its own amplitudes: t1 and t2 must be NULL");
    if (kind != TF_TRIPLES_MP4 && (!t1 || !t2)) TF_FAIL(ctx, TF_EINVAL, "tf_triples_rhf: CCSD(T) and QCISD(T) need t1 and t2");
    const int N = S.N, o = S.o, v = S.v;
    const long long ov = S.ov, B2 = S.B2;
    if (ov > 0x7fffffffLL || (long long)o * v * v > 0x7fffffffLL) TF_FAIL(ctx, TF_EINVAL, "tf_triples_rhf: dimension overflow");
    const size_t v2 = (size_t)v * v, v3 = v2 * v, o3 = (size_t)o * o * o;
    const long long n_triples = (long long)o * (o + 1) * (o + 2) / 6 - o;
    out->e_t = out->e_connected = out->e_disconnected = 0.0;
    out->n_triples = n_triples;
    for (int q = 0; q < 4; ++q) out->seconds[q] = 0.0;
    const std::vector<double> &Co = S.Co, &Cv = S.Cv;
    DeviceBlocks mem;
    auto fail = [&](int code, const std::string &m) { return corr_fail(ctx, code, m); };
    // ---- the resident arrays: (ia|bc), the six X, t2; small: partials [2 n_blocks] | per-triple sums [2 n_triples] | eps [N] | t1 [ov]
    const int nt = (v + tftriples::TT - 1) / tftriples::TT;
    const long long n_blocks = (long long)nt * (nt + 1) * (nt + 2) / 6;
    const size_t nsmall = 2 * (size_t)n_blocks + 2 * (size_t)std::max<long long>(1, n_triples) + (size_t)N + (size_t)ov;
    double *gv = mem.alloc((size_t)o * v3), *X = gv ? mem.alloc(6 * v3) : nullptr, *d_t2 = X ? mem.alloc((size_t)B2) : nullptr,
           *d_small = d_t2 ? mem.alloc(nsmall) : nullptr;
    int *d_tiles = d_small ? mem.alloc_int((size_t)3 * n_blocks) : nullptr;
    if (!d_tiles) {
        char text[200];
        snprintf(text, sizeof text, "tf_triples_rhf: out of device memory for %.2f GB of work space ((ia|bc): o v^3 values, six arrays of v^3 and t2)",
                 (double)((size_t)o * v3 + 6 * v3 + (size_t)B2 + nsmall) * sizeof(double) / 1e9);
        return fail(TF_ENOMEM, text);
    }
    double *d_part = d_small, *d_e = d_part + 2 * (size_t)n_blocks, *d_eps = d_e + 2 * (size_t)std::max<long long>(1, n_triples), *d_t1 = d_eps + N;
    // ---- MO blocks: (ia|jb) = g1[i][a][j][b], (ki|ld) = g4[k][i][l][d], (ia|bc) = gv[i][a][b][c]
    double *g1 = nullptr, *g4 = nullptr;
    if ((rc = mo_transform_device(ctx, Co.data(), o, Cv.data(), v, Co.data(), o, Cv.data(), v, mem, &g1, nullptr))) return rc;
    if ((rc = mo_transform_device(ctx, Co.data(), o, Co.data(), o, Co.data(), o, Cv.data(), v, mem, &g4, nullptr))) return rc;
    {
        // the transformation's scratch is about 1.5 N^2 values per element of the ket pair, for both images of a packed tensor: (slab, v) and
        // (slice of b, v).  A quarter of the free memory, 32 GB at the most, bounds either.
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return fail(TF_ENODEVICE, "tf_triples_rhf: hipMemGetInfo failed");
        const size_t budget = std::min<size_t>((free_b + tfcache::cached()) / 4, (size_t)32 << 30);
        const long long cap = std::max<long long>(1, (long long)(budget / ((size_t)12 * N * N * v)));
        long long slab = std::min<long long>(o, cap);
        if (const char *env = getenv("TF_TRIPLES_SLAB")) { const long long n = atoll(env); if (n >= 1) slab = std::min(slab, n); }
        long long slice = std::min<long long>(v, cap);
        if (const char *env = getenv("TF_TRIPLES_SLICE")) { const long long n = atoll(env); if (n >= 1) slice = std::min(slice, n); }
        const int nb_max = (int)slice;
        std::vector<double> Cos((size_t)N * slab), Cs((size_t)N * nb_max);
        for (int i0 = 0; i0 < o; i0 += (int)slab) {
            const int ns = (int)std::min<long long>(slab, o - i0);
            column_window(Co.data(), N, o, i0, ns, Cos.data());
            for (int b0 = 0; b0 < v; b0 += nb_max) {
                const int nb = std::min(nb_max, v - b0);
                column_window(Cv.data(), N, v, b0, nb, Cs.data());
                DeviceBlocks part;
                double *d_s = nullptr;
                if ((rc = mo_transform_device(ctx, Cos.data(), ns, Cv.data(), v, Cs.data(), nb, Cv.data(), v, part, &d_s, nullptr))) return rc;
                // [is][a][b'][c] -> gv[i0 + is][a][b0 + b'][c]: ns v rows of nb v values, v^2 apart
                if (hipMemcpy2D(gv + (size_t)i0 * v3 + (size_t)b0 * v, v2 * sizeof(double), d_s, (size_t)nb * v * sizeof(double), (size_t)nb * v * sizeof(double),
                                (size_t)ns * v, hipMemcpyDeviceToDevice) != hipSuccess)
                    return fail(TF_ENODEVICE, "tf_triples_rhf: copy failed");
            }
        }
    }
    const auto t1s = corr_stamp();
    // ---- amplitudes, orbital energies, the tile triples t0 <= t1 <= t2
    {
        std::vector<int> tiles((size_t)3 * n_blocks);
        size_t n = 0;
        for (int a = 0; a < nt; ++a)
            for (int b = a; b < nt; ++b)
                for (int c = b; c < nt; ++c) { tiles[n++] = a; tiles[n++] = b; tiles[n++] = c; }
        if (hipMemcpy(d_tiles, tiles.data(), tiles.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_eps, eps, (size_t)N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
            return fail(TF_ENODEVICE, "tf_triples_rhf: copy failed");
    }
    if (kind == TF_TRIPLES_MP4) {
        hipLaunchKernelGGL(tftriples::triples_mp2_amplitudes_kernel, dim3((unsigned)std::min<long long>((B2 + 255) / 256, 1 << 16)), dim3(256), 0, 0, g1, d_eps,
                           n_frozen, n_occ, o, v, d_t2);
    } else if (hipMemcpy(d_t2, t2, (size_t)B2 * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
               hipMemcpy(d_t1, t1, (size_t)ov * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return fail(TF_ENODEVICE, "tf_triples_rhf: copy failed");
    // ---- the loop over unordered triples.  Split-K GEMM kernels would change their sums from run to run
    rocblas_handle blas = ctx->scf.blas;
    BlasAtomicsOff no_atomics(blas);
    static const int P3[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};    // tftriples::perm3
    const auto t2s = corr_stamp();
    {
        tftriples::EnergyArgs A{};
        for (int n = 0; n < 6; ++n) A.X[n] = X + (size_t)n * v3;
        A.tiles = d_tiles; A.g1 = g1; A.t1 = d_t1; A.eps = d_eps;
        A.vscale = kind == TF_TRIPLES_CCSD_T ? 1.0 : (kind == TF_TRIPLES_QCISD_T ? 2.0 : 0.0);
        A.n_frozen = n_frozen; A.n_occ = n_occ; A.o = o; A.v = v; A.partial = d_part;
        long long t = 0;
        for (int i = 0; i < o; ++i)
            for (int j = 0; j <= i; ++j)
                for (int k = 0; k <= j; ++k) {
                    if (i == k) continue;
                    const int occ[3] = {i, j, k};
                    for (int n = 0; n < 6; ++n) {
                        const int p = occ[P3[n][0]], q = occ[P3[n][1]], r = occ[P3[n][2]];
                        double *Xn = X + (size_t)n * v3;
                        // X[(ab)][c] = (pa|b.) [v^2 x v] t2[r,q]^T;  X[a][(bc)] -= (pa|q.) [v x o] t2[.,r] [o x v^2]
                        CORR_BLAS(tfmp3::gemm_rm(blas, false, true, (int)v2, v, v, 1.0, gv + (size_t)p * v3, v, d_t2 + ((size_t)r * o + q) * v2, v, 0.0, Xn, v));
                        CORR_BLAS(tfmp3::gemm_rm(blas, true, false, v, (int)v2, o, -1.0, g4 + ((size_t)q * o * o + p) * v, (int)ov, d_t2 + (size_t)r * v2,
                                                 (int)((size_t)o * v2), 1.0, Xn, (int)v2));
                    }
                    A.i = i; A.j = j; A.k = k;
                    hipLaunchKernelGGL(tftriples::triples_energy_kernel, dim3((unsigned)n_blocks), dim3(tftriples::THREADS), 0, 0, A);
                    hipLaunchKernelGGL(tftriples::triples_sum_partials_kernel, dim3(1), dim3(tftriples::THREADS), 0, 0, d_part, (int)n_blocks, d_e + 2 * t);
                    ++t;
                }
    }
    if (hipGetLastError() != hipSuccess) return fail(TF_ENODEVICE, "tf_triples_rhf: a kernel launch failed");
    std::vector<double> e2(2 * (size_t)std::max<long long>(1, n_triples), 0.0);
    if (n_triples > 0 && hipMemcpy(e2.data(), d_e, 2 * (size_t)n_triples * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(TF_ENODEVICE, "tf_triples_rhf: the triples kernels failed on the device");
    const auto t3s = corr_stamp();
    if (out->e_ijk) std::fill(out->e_ijk, out->e_ijk + o3, 0.0);
    {
        double ec = 0.0, ed = 0.0;
        long long t = 0;
        for (int i = 0; i < o; ++i)
            for (int j = 0; j <= i; ++j)
                for (int k = 0; k <= j; ++k) {
                    if (i == k) continue;
                    const double c = e2[2 * t] / 3.0, d = e2[2 * t + 1] / 3.0, w = (i == j || j == k) ? 3.0 : 6.0;
                    ec += w * c; ed += w * d;
                    if (out->e_ijk) {
                        const int occ[3] = {i, j, k};
                        for (int n = 0; n < 6; ++n)
                            out->e_ijk[((size_t)occ[P3[n][0]] * o + occ[P3[n][1]]) * o + occ[P3[n][2]]] = c + d;
                    }
                    ++t;
                }
        out->e_connected = ec; out->e_disconnected = ed; out->e_t = ec + ed;
    }
    mem.clear();                                              // the wall time includes the release, as it always has
    const auto t4 = std::chrono::steady_clock::now();
    out->seconds[0] = corr_secs(t4 - S.t0);
    out->seconds[1] = corr_secs(t1s - S.t0);
    out->seconds[2] = corr_secs(t3s - t2s);
    out->seconds[3] = out->seconds[0] - out->seconds[1] - out->seconds[2];
    return TF_OK;
}

// The restricted MP2 one-particle density, unrelaxed or Z-vector relaxed (run_restricted_MP2, tuna_mp.py:908-966;
// calculate_restricted_relaxed_MP2_density_matrix, :177-279; tf_mp2dens.hip.h has the expressions).  Stages: the MO blocks (ia|jb) and,
// relaxed, (ab|ij) and (ji|kb) through mo_transform_device; the amplitudes and the MP2 partials (mp2dens_amp_kernel); the unrelaxed blocks
// as four GEMMs; relaxed: one pass of mp3_ladder_stage on w with the occupied back-transformation (tf_mp4_rhf's singles), o GEMMs over
// (ji|kb), one J/K build of C P^(2) C^T, the Lagrangian (mp2dens_lagrangian_kernel), A + B by tf_cis_rhf's assembly pass, dpotrf and
// dpotrs.  Work space of a relaxed call: at most 6 arrays of o^2 v^2 values at a time ((ia|jb), (ab|ij), tOS, tSS, w in two layouts; tOS
// and tSS are freed before the ladder's Y comes, w before the transposed (ij|ab) and the (o v)^2 of A + B); an unrelaxed call has 3.
int tf_mp2_density_rhf(tf_ctx *ctx, const tf_mp2_density_opts *opts, int n_occ, int n_frozen, const double *C, const double *eps,
                       tf_mp2_density_result *out)
{
    static const char *who = "tf_mp2_density_rhf";
    int rc = corr_args(ctx, who, opts && C && eps && out, " (needs opts, C, eps, out and 0 <= n_frozen < n_occ < N)", n_occ, n_frozen);
    if (rc) return rc;
    const bool relaxed = opts->relaxed != 0;
    if (relaxed && n_frozen != 0)
        TF_FAIL(ctx, TF_EINVAL, "tf_mp2_density_rhf: the relaxed density needs n_frozen = 0, got %d: the frozen-core Z-vector equations (A over all "
                "occupied orbitals, B over the active ones) are not built; the unrelaxed density takes a frozen core", n_frozen);
    if (relaxed && !out->P_mo && !out->P_ao && !out->L && !out->z) TF_FAIL(ctx, TF_EINVAL, "tf_mp2_density_rhf: a relaxed call needs one of P_mo, P_ao, L, z");
    CorrSetup S;
    if ((rc = corr_begin(ctx, who, n_occ, n_frozen, C, S))) return rc;
    const int N = S.N, o = S.o, v = S.v;
    const long long ov = S.ov, B2 = S.B2, o3v = (long long)o * o * ov;
    if (ov > 2000000LL || (long long)v * v > 2000000LL || ov * (long long)std::max(o, v) > 0x7fffffffLL) TF_FAIL(ctx, TF_EINVAL, "tf_mp2_density_rhf: dimension overflow");
    const int dim = (int)ov, iov = dim;
    const size_t nn = (size_t)N * N;
    DeviceBlocks mem;
    auto fail = [&](int code, const std::string &m) { return corr_fail(ctx, code, m); };
    // ---- MO blocks: (ia|jb) = g1[i][a][j][b]; relaxed: (ab|ij) = g2[a][b][i][j] and (ji|kb) = g4[j][i][k][b]
    double *g1 = nullptr, *g2 = nullptr, *g4 = nullptr;
    if ((rc = mo_transform_device(ctx, S.Co.data(), o, S.Cv.data(), v, S.Co.data(), o, S.Cv.data(), v, mem, &g1, nullptr))) return rc;
    if (relaxed) {
        if (!(g2 = mem.alloc((size_t)B2))) return fail(TF_ENOMEM, "tf_mp2_density_rhf: out of device memory");
        if ((rc = mo_vvoo_block(ctx, who, S.Cv, S.Cv, S.Co, S.Co, o, v, g2))) return rc;
        if ((rc = mo_transform_device(ctx, S.Co.data(), o, S.Co.data(), o, S.Co.data(), o, S.Cv.data(), v, mem, &g4, nullptr))) return rc;
    }
    const auto t1 = corr_stamp();
    // ---- work space.  amps: tOS | tSS; ww: w[i][a][j][b] | w[i][j][a][b]; small: partials [2 nblk] | Poo [o^2] | Pvv [v^2] | C [N^2] |
    //      P2 (MO) [N^2] | P_mo [N^2] | T [N^2] | P_ao [N^2], and relaxed J | K | P_src [N^2 each] | T1 [N v] | L2 | Lf | L | z [o v each] |
    //      OA | OB [o^3 v each] | Vo [TFL_W N o]
    const int nblk = CORR_NBLK;
    const size_t nsmall = (size_t)2 * nblk + (size_t)o * o + (size_t)v * v + 5 * nn +
                          (relaxed ? 3 * nn + (size_t)N * v + 4 * (size_t)ov + 2 * (size_t)o3v + (size_t)TFL_W * N * o : 0);
    const size_t nladder = relaxed ? mp3_ladder_work_doubles(ctx, v) : 0;
    char oom[220];
    snprintf(oom, sizeof oom, "tf_mp2_density_rhf: out of device memory for %.2f GB of work space (%s)",
             (double)((relaxed ? 6 : 3) * (size_t)B2 + nsmall + nladder) * sizeof(double) / 1e9,
             relaxed ? "6 arrays of o^2 v^2 values at a time, (o v)^2 for A + B among them, and the ladder's batch" : "3 arrays of o^2 v^2 values");
    double *amps = mem.alloc(2 * (size_t)B2), *ww = relaxed ? mem.alloc(2 * (size_t)B2) : nullptr, *small = mem.alloc(nsmall);
    if (!amps || (relaxed && !ww) || !small) return fail(TF_ENOMEM, oom);
    double *tos = amps, *tss = amps + B2, *wov = ww, *woo = ww ? ww + B2 : nullptr;
    double *d_part = small, *Poo = d_part + (size_t)2 * nblk, *Pvv = Poo + (size_t)o * o, *dC = Pvv + (size_t)v * v, *P2 = dC + nn, *Pmo = P2 + nn, *Tn = Pmo + nn,
           *Pao = Tn + nn, *dJ = Pao + nn, *dK = dJ + nn, *Psrc = dK + nn, *T1 = Psrc + nn, *L2 = T1 + (size_t)N * v, *Lf = L2 + ov, *dL = Lf + ov, *dz = dL + ov,
           *OA = dz + ov, *OB = OA + o3v, *Vo = OB + o3v;
    if ((rc = corr_upload(ctx, who, S, mem, eps, nullptr, relaxed, oom))) return rc;
    if (hipMemcpy(dC, C, nn * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return fail(TF_ENODEVICE, "tf_mp2_density_rhf: copy failed");
    rocblas_handle blas = ctx->scf.blas;
    BlasAtomicsOff no_atomics(blas);                          // no split-K sums: the same call gives the same bits
    // ---- amplitudes and the MP2 partials
    hipLaunchKernelGGL(tfmp2dens::mp2dens_amp_kernel, dim3(nblk), dim3(256), 0, 0, g1, S.d_eps, n_frozen, o, v, n_occ, opts->c_os, opts->c_ss, tos, tss, wov, woo,
                       d_part);
    double e2[2];
    if (sum_partials_host(d_part, nblk, 2, e2) != hipSuccess) return fail(TF_ENODEVICE, "tf_mp2_density_rhf: the amplitude kernel failed on the device");
    out->e_os = e2[0]; out->e_ss = e2[1];
    // ---- unrelaxed: Poo = -1/2 c_os TOS TOS^T - c_ss TSS TSS^T with T [o][(v o v)]; Pvv = 1/2 c_os MOS^T MOS + c_ss MSS^T MSS with M [(o v o)][v]
    const int vov = v * iov, ovo = o * iov;
    CORR_BLAS(tfmp3::gemm_rm(blas, false, true, o, o, vov, -0.5 * opts->c_os, tos, vov, tos, vov, 0.0, Poo, o));
    CORR_BLAS(tfmp3::gemm_rm(blas, false, true, o, o, vov, -opts->c_ss, tss, vov, tss, vov, 1.0, Poo, o));
    CORR_BLAS(tfmp3::gemm_rm(blas, true, false, v, v, ovo, 0.5 * opts->c_os, tos, v, tos, v, 0.0, Pvv, v));
    CORR_BLAS(tfmp3::gemm_rm(blas, true, false, v, v, ovo, opts->c_ss, tss, v, tss, v, 1.0, Pvv, v));
    const dim3 grid_nn((unsigned)((nn + 255) / 256));
    hipLaunchKernelGGL(tfmp2dens::mp2dens_assemble_kernel, grid_nn, dim3(256), 0, 0, Poo, Pvv, (const double *)nullptr, 0, N, n_frozen, n_occ, P2);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(TF_ENODEVICE, "tf_mp2_density_rhf: the unrelaxed stage failed on the device");
    mem.release(amps);
    auto t2 = corr_stamp(), t3 = t2, t4 = t2, t5 = t2;
    if (relaxed) {
        // ---- Lagrangian, first term: one ladder pass on w with the occupied back-transformation (OA, OB)
        double *Y = mem.alloc((size_t)B2), *batch = Y ? mem.alloc(nladder) : nullptr;
        if (!batch) return fail(TF_ENOMEM, oom);
        corr_permute(ctx, S);
        if ((rc = mp3_ladder_stage(ctx, who, o, v, woo, S.Cvl, batch, Y, S.Col, Vo, OA, OB))) return rc;
        t3 = corr_stamp();
        mem.release(batch); mem.release(Y);
        // ---- second term: L2[i][a] = sum_j sum_(kb) (ji|kb) w[j][a][(kb)]
        for (int j = 0; j < o; ++j)
            CORR_BLAS(tfmp3::gemm_rm(blas, false, true, o, v, iov, 1.0, g4 + (size_t)j * o * ov, iov, wov + (size_t)j * v * ov, iov, j ? 1.0 : 0.0, L2, v));
        // ---- Fock response: P_src = sym(C P2 C^T), Lf = C_o^T (4 J - 2 K) C_v
        CORR_BLAS(tfmp3::gemm_rm(blas, false, false, N, N, N, 1.0, dC, N, P2, N, 0.0, Tn, N));
        CORR_BLAS(tfmp3::gemm_rm(blas, false, true, N, N, N, 1.0, Tn, N, dC, N, 0.0, Pao, N));
        hipLaunchKernelGGL(tfscf::k_symmetrise, grid_nn, dim3(256), 0, 0, Pao, Psrc, N);
        {
            const double *pp[8]; double *jj[8], *kk[8];
            for (int q = 0; q < 8; ++q) { pp[q] = Psrc; jj[q] = dJ; kk[q] = dK; }
            if ((rc = launch_jk(ctx, 1, pp, jj, kk, 0))) return rc;
        }
        CORR_BLAS(tfmp3::gemm_rm(blas, false, false, N, v, N, 4.0, dJ, N, S.d_Cv, v, 0.0, T1, v));
        CORR_BLAS(tfmp3::gemm_rm(blas, false, false, N, v, N, -2.0, dK, N, S.d_Cv, v, 1.0, T1, v));
        CORR_BLAS(tfmp3::gemm_rm(blas, true, false, o, v, N, 1.0, S.d_Co, o, T1, v, 0.0, Lf, v));
        hipLaunchKernelGGL(tfmp2dens::mp2dens_lagrangian_kernel, dim3((unsigned)((ov + 255) / 256)), dim3(256), 0, 0, OA, OB, S.packed ? 1 : 0, L2, Lf, o, v, dL, dz);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(TF_ENODEVICE, "tf_mp2_density_rhf: the Lagrangian stage failed on the device");
        mem.release(ww);
        t4 = corr_stamp();
        // ---- Z-vector: (A + B) z = -L
        double *Ht = mem.alloc((size_t)B2), *M = Ht ? mem.alloc((size_t)B2) : nullptr;
        rocblas_int *d_info = M ? mem.alloc_int(4) : nullptr;
        if (!d_info) return fail(TF_ENOMEM, oom);
        tfcis::launch_transpose(g2, (long long)v * v, (long long)o * o, Ht, 0);
        {
            tfcis::AssembleArgs A{};
            A.g1 = g1; A.Ht = Ht; A.eps = S.d_eps; A.n_frozen = n_frozen; A.n_occ = n_occ; A.o = o; A.v = v;
            A.kind[0] = 2; A.out[0] = M; A.n_out = 1;
            tfcis::launch_assemble(A, 0);
        }
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(TF_ENODEVICE, "tf_mp2_density_rhf: the assembly kernels failed on the device");
        mem.release(Ht);
        CORR_BLAS_WHAT("rocSOLVER", rocsolver_dpotrf(blas, rocblas_fill_lower, dim, M, dim, d_info));
        int h = 0;
        if (hipMemcpy(&h, d_info, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return fail(TF_ENODEVICE, "tf_mp2_density_rhf: the Cholesky factorisation failed on the device");
        if (h != 0) {
            char text[320];
            snprintf(text, sizeof text, "tf_mp2_density_rhf: A + B is not positive definite (dpotrf stopped at the leading minor of order %d of %d): the RHF "
                     "solution is singlet-unstable, the Z-vector equations have no meaningful solution and no relaxed density is returned", h, dim);
            return fail(TF_ELINALG, text);
        }
        CORR_BLAS_WHAT("rocSOLVER", rocsolver_dpotrs(blas, rocblas_fill_lower, dim, 1, M, dim, dz, dim));
        t5 = corr_stamp();
    }
    // ---- P_mo with the reference determinant's 2 on the occupied diagonal, P_ao = C P_mo C^T
    hipLaunchKernelGGL(tfmp2dens::mp2dens_assemble_kernel, grid_nn, dim3(256), 0, 0, Poo, Pvv, relaxed ? (const double *)dz : (const double *)nullptr, 1, N, n_frozen,
                       n_occ, Pmo);
    CORR_BLAS(tfmp3::gemm_rm(blas, false, false, N, N, N, 1.0, dC, N, Pmo, N, 0.0, Tn, N));
    CORR_BLAS(tfmp3::gemm_rm(blas, false, true, N, N, N, 1.0, Tn, N, dC, N, 0.0, Pao, N));
    if ((out->P_mo && hipMemcpy(out->P_mo, Pmo, nn * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) ||
        (out->P_ao && hipMemcpy(out->P_ao, Pao, nn * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) ||
        (relaxed && out->L && hipMemcpy(out->L, dL, (size_t)ov * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) ||
        (relaxed && out->z && hipMemcpy(out->z, dz, (size_t)ov * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) || hipGetLastError() != hipSuccess)
        return fail(TF_ENODEVICE, "tf_mp2_density_rhf: the density kernels or the copies failed on the device");
    const auto t6 = corr_stamp();
    out->seconds[0] = corr_secs(t6 - S.t0);
    out->seconds[1] = corr_secs(t1 - S.t0);
    out->seconds[2] = corr_secs(t3 - t2);
    out->seconds[3] = corr_secs(t5 - t4);
    out->seconds[4] = out->seconds[0] - out->seconds[1] - out->seconds[2] - out->seconds[3];
    return TF_OK;
}

// Natural orbitals of a density matrix P [n][n] in a basis with orthogonaliser X (calculate_natural_orbitals, tuna_mp.py:514-565): the
// eigenpairs of X^-1 P X^-T by the context's eigensolver (X^-1 by dgetrf / dgetri), occupations descending, orbitals = X vectors.
int tf_natural_orbitals(tf_ctx *ctx, int n, const double *P, const double *X, double *occ, double *orbitals)
{
    static const char *who = "tf_natural_orbitals";
    if (!ctx) return TF_EINVAL;
    if (n < 1 || !P || !X || !occ || !orbitals) TF_FAIL(ctx, TF_EINVAL, "tf_natural_orbitals: bad arguments (needs n >= 1, P, X, occ and orbitals)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::string msg;
    int rc = tfscf::ensure(ctx->scf, n, 6, msg);
    if (rc) { ctx->err = msg; return rc; }
    offer_symmetry(ctx, ctx->scf, n);
    const size_t nn = (size_t)n * n;
    DeviceBlocks mem;
    double *buf = mem.alloc(6 * nn + 5 * (size_t)n);           // X | X^-1 | P | T | W | orbitals, then vals | work [3 n] | occ
    rocblas_int *ipiv = buf ? mem.alloc_int((size_t)n + 4) : nullptr;
    if (!ipiv) TF_FAIL(ctx, TF_ENOMEM, "tf_natural_orbitals: out of device memory");
    rocblas_int *d_info = ipiv + n;
    double *dX = buf, *dXi = dX + nn, *dP = dXi + nn, *T = dP + nn, *W = T + nn, *dO = W + nn, *vals = dO + nn, *work = vals + n, *d_occ = work + 3 * (size_t)n;
    if (hipMemcpy(dX, X, nn * sizeof(double), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dXi, X, nn * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dP, P, nn * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return corr_fail(ctx, TF_ENODEVICE, "tf_natural_orbitals: copy failed");
    rocblas_handle blas = ctx->scf.blas;
    BlasAtomicsOff no_atomics(blas);
    // the inverse of a row-major matrix is the row-major reading of the inverse of its column-major reading
    CORR_BLAS_WHAT("rocSOLVER", rocsolver_dgetrf(blas, n, n, dXi, n, ipiv, d_info));
    int h = 0;
    if (hipMemcpy(&h, d_info, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return corr_fail(ctx, TF_ENODEVICE, "tf_natural_orbitals: the factorisation failed on the device");
    if (h != 0) TF_FAIL(ctx, TF_ELINALG, "tf_natural_orbitals: X is singular (dgetrf found a zero pivot at %d of %d)", h, n);
    CORR_BLAS_WHAT("rocSOLVER", rocsolver_dgetri(blas, n, dXi, n, ipiv, d_info));
    CORR_BLAS(tfmp3::gemm_rm(blas, false, false, n, n, n, 1.0, dXi, n, dP, n, 0.0, T, n));
    CORR_BLAS(tfmp3::gemm_rm(blas, false, true, n, n, n, 1.0, T, n, dXi, n, 0.0, dO, n));
    hipLaunchKernelGGL(tfscf::k_symmetrise, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, 0, dO, W, n);
    if ((rc = tfscf::eigh(ctx->scf, n, W, vals, work, msg))) { ctx->err = msg; return rc; }
    // the solver's vectors are the rows of W: X W^T has them as columns, in ascending order
    CORR_BLAS(tfmp3::gemm_rm(blas, false, true, n, n, n, 1.0, dX, n, W, n, 0.0, T, n));
    hipLaunchKernelGGL(tfmp2dens::natorb_reverse_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, 0, vals, T, n, d_occ, dO);
    if (hipMemcpy(occ, d_occ, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(orbitals, dO, nn * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess || hipGetLastError() != hipSuccess)
        return corr_fail(ctx, TF_ENODEVICE, "tf_natural_orbitals: the kernels or the copies failed on the device");
    return TF_OK;
}

int tf_mp3_ladder_probe(tf_ctx *ctx, int n, const double *T, double *Zh)
{
    if (!ctx) return TF_EINVAL;
    if (!ctx->have_eri) TF_FAIL(ctx, TF_EINVAL, "tf_mp3_ladder_probe: call tf_build_eri first");
    if (n < 1 || !T || !Zh) TF_FAIL(ctx, TF_EINVAL, "tf_mp3_ladder_probe: bad arguments (needs n >= 1, T and Zh)");
    if (ctx->world > 1) TF_FAIL(ctx, TF_EINVAL, "tf_mp3_ladder_probe: a sharded tensor (world > 1) is not supported");
    if (ctx->layout != 1) TF_FAIL(ctx, TF_EINVAL, "tf_mp3_ladder_probe: the ladder kernel runs on the packed layout only");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int N = ctx->N, W = TFL_W;
    const size_t nn = (size_t)N * N, nT = (size_t)W * nn;
    const int *oI = ctx->hl.origI.data();                     // internal -> caller's AO index
    DeviceBlocks mem;
    double *buf = mem.alloc(3 * nT);                          // T [W][N][N] | Tt [N][N][W] | Zh [W][N][N]
    if (!buf) TF_FAIL(ctx, TF_ENOMEM, "tf_mp3_ladder_probe: out of device memory");
    auto fail = [&](int code, const char *m) { return corr_fail(ctx, code, m); };
    double *Tm = buf, *Tt = Tm + nT, *Zd = Tt + nT;
    std::vector<double> h(nT);
    for (int p0 = 0; p0 < n; p0 += W) {
        const int nb = std::min(W, n - p0);
        for (int p = 0; p < nb; ++p)
            for (int x = 0; x < N; ++x) {
                const double *src = T + (size_t)(p0 + p) * nn + (size_t)oI[x] * N;
                double *dst = h.data() + (size_t)p * nn + (size_t)x * N;
                for (int y = 0; y < N; ++y) dst[y] = src[oI[y]];
            }
        // every byte of the output 0xff first: an element the kernel does not write comes back as a NaN
        if (hipMemcpy(Tm, h.data(), (size_t)nb * nn * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemset(Zd, 0xff, nT * sizeof(double)) != hipSuccess)
            return fail(TF_ENODEVICE, "tf_mp3_ladder_probe: copy failed");
        if (!mp3_ladder_batch(ctx, Tm, nb, Tt, Zd)) return fail(TF_ENODEVICE, "tf_mp3_ladder_probe: ladder kernel launch failed");
        if (hipMemcpy(h.data(), Zd, (size_t)nb * nn * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
            return fail(TF_ENODEVICE, "tf_mp3_ladder_probe: the ladder kernel failed on the device");
        for (int p = 0; p < nb; ++p)
            for (int x = 0; x < N; ++x) {
                const double *src = h.data() + (size_t)p * nn + (size_t)x * N;
                double *dst = Zh + (size_t)(p0 + p) * nn + (size_t)oI[x] * N;
                for (int y = 0; y < N; ++y) dst[oI[y]] = src[y];
            }
    }
    return TF_OK;
}

