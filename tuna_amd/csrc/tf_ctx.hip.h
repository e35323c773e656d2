// tf_ctx.hip.h -- what every host unit of libtunafock stands on: the small-block cache behind tf_malloc / tf_free,
// the owners of device memory, struct tf_ctx, the failure macros, upload, and free_eri / free_basis.  Included by tf_device.hip below
// the kernel headers and above every other host unit; one translation unit.  Three lifetimes and one owner each:
//   context  tf_ctx::blk (tfctx::CtxBlock, tf_ctx_plan.h), bstreams, prof, comm      released by tf_destroy
//   basis    tf_ctx::basis_mem and what tf_set_basis commits with it                   released by free_basis
//   build    tf_ctx::build_mem and the views into it (jk, tv, bl, d_row*)              released by free_eri

// ---- small-block cache for THIS file's device allocations ------------------------------------------------------------------------
// A tensor build uploads ~40 small tables (layout, rows, work lists) and frees them again; every hipMalloc / hipFree pair costs 20-40 us
// of host time and hipFree synchronises the device -- at N = 60 that is a third of the 3.3 ms a build takes.  Blocks of up to 64 MiB are
// therefore recycled: size classes of powers of two (>= 512 bytes), at most 1 GiB kept; larger blocks and unknown pointers go straight
// to the runtime.  What hipFree's implicit synchronisation used to guarantee -- no kernel still reads a block that is handed out
// again -- is kept by the explicit hipDeviceSynchronize() in free_eri / free_basis (the two places that free buffers kernels of
// EARLIER calls may still use).  Per process and device, mutex-protected (the lockstep SCF batch runs on several host threads).
namespace tfcache {
struct Block { void *p; int dev; };
static std::mutex mu;
static std::multimap<size_t, Block> free_blocks;            // size class -> cached block
static std::map<void *, std::pair<size_t, int>> live;       // blocks handed out by cmalloc: (size class, device)
static size_t cached_bytes = 0;
static const size_t MAX_BLOCK = (size_t)64 << 20, MAX_CACHED = (size_t)1 << 30;
static const bool off = getenv("TF_ALLOC_CACHE") && getenv("TF_ALLOC_CACHE")[0] == '0';
static size_t size_class(size_t b) { size_t c = 512; while (c < b) c <<= 1; return c; }
// Hands every cached block back to the runtime (after a device-wide synchronisation: a kernel of an earlier call may still read one).
// Called when the runtime is out of memory -- the cache must never be the reason a build fails -- and by tf_destroy of the last context.
static void trim()
{
    std::lock_guard<std::mutex> lk(mu);
    if (free_blocks.empty()) return;
    int dev0 = 0;
    (void)hipGetDevice(&dev0);
    for (auto &kv : free_blocks) {
        (void)hipSetDevice(kv.second.dev);
        (void)hipDeviceSynchronize();
        (void)::hipFree(kv.second.p);
    }
    (void)hipSetDevice(dev0);
    free_blocks.clear();
    cached_bytes = 0;
}
static size_t cached() { std::lock_guard<std::mutex> lk(mu); return cached_bytes; }
static hipError_t raw_malloc(void **p, size_t bytes)
{
    hipError_t e = ::hipMalloc(p, bytes);
    if (e == hipErrorOutOfMemory && cached() > 0) {
        (void)hipGetLastError();
        trim();
        e = ::hipMalloc(p, bytes);
    }
    return e;
}
static hipError_t cmalloc(void **p, size_t bytes)
{
    if (off || bytes > MAX_BLOCK) return raw_malloc(p, bytes);
    int dev = 0;
    (void)hipGetDevice(&dev);
    const size_t c = size_class(bytes);
    {
        std::lock_guard<std::mutex> lk(mu);
        auto range = free_blocks.equal_range(c);
        for (auto it = range.first; it != range.second; ++it)
            if (it->second.dev == dev) {
                *p = it->second.p;
                free_blocks.erase(it);
                cached_bytes -= c;
                live[*p] = std::make_pair(c, dev);
                return hipSuccess;
            }
    }
    hipError_t e = raw_malloc(p, c);
    if (e == hipSuccess) { std::lock_guard<std::mutex> lk(mu); live[*p] = std::make_pair(c, dev); }
    return e;
}
static thread_local bool bypass = false;     // set while blocks are released after a failed synchronisation: straight back to the runtime
static hipError_t cfree(void *p)
{
    if (!p) return hipSuccess;
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = live.find(p);
        if (it != live.end()) {
            const size_t c = it->second.first;
            const int dev = it->second.second;
            live.erase(it);
            if (!bypass && cached_bytes + c <= MAX_CACHED) {
                free_blocks.emplace(c, Block{p, dev});
                cached_bytes += c;
                return hipSuccess;
            }
        }
    }
    return ::hipFree(p);
}
}  // namespace tfcache
// every device allocation of this file goes through the cache (blocks released elsewhere with the runtime's hipFree use ::hipMalloc)
static inline hipError_t tf_malloc(void **p, size_t bytes) { return tfcache::cmalloc(p, bytes); }
template <class T> static inline hipError_t tf_malloc(T **p, size_t bytes) { return tfcache::cmalloc((void **)p, bytes); }
static inline hipError_t tf_free(void *p) { return tfcache::cfree(p); }

// Owner of device allocations with one lifetime -- one call of a post-SCF driver (tf_corr_host.hip.h), one tensor build (tf_ctx::build_mem):
// whatever it still holds is freed, in the order it was handed out, by clear() and when the owner goes out of scope.  A block is freed
// through its owner only, so no pointer can reach the cache twice.
struct __attribute__((visibility("hidden"))) DeviceBlocks {
    std::vector<void *> held;
    DeviceBlocks() = default;
    DeviceBlocks(const DeviceBlocks &) = delete;
    DeviceBlocks &operator=(const DeviceBlocks &) = delete;
    ~DeviceBlocks() { clear(); }
    hipError_t take(void **p, size_t bytes)                   // tf_malloc into *p; the block is held from then on
    {
        const hipError_t e = tf_malloc(p, bytes);
        if (e == hipSuccess) held.push_back(*p);
        return e;
    }
    void *alloc_bytes(size_t bytes)                           // nullptr: out of device memory
    {
        void *p = nullptr;
        if (take(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        return p;
    }
    double *alloc(size_t n) { return (double *)alloc_bytes(n * sizeof(double)); }
    int *alloc_int(size_t n) { return (int *)alloc_bytes(n * sizeof(int)); }   // (rocblas_int is int)
    void release(void *p)                                     // early free of one block (a null or foreign pointer is left alone)
    {
        const auto it = std::find(held.begin(), held.end(), p);
        if (p && it != held.end()) { (void)tf_free(p); held.erase(it); }
    }
    void clear() { for (void *p : held) (void)tf_free(p); held.clear(); }
};

using namespace tfk;

static std::string g_create_error;
static std::atomic<int> g_live_contexts{0};
static const bool g_dbg = getenv("TF_DEBUG") != nullptr;
static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
#define DBG(...) do { if (g_dbg) { fprintf(stderr, "[tf %.6f] ", now_s()); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); fflush(stderr); } } while (0)

// the runtime behind the owners of tf_ctx_plan.h (codes are hipError_t values)
static int ctx_dev_alloc(void **p, size_t bytes) { return (int)tf_malloc(p, bytes); }
static void ctx_dev_free(void *p) { (void)tf_free(p); }
struct HipHandles {
    typedef hipStream_t Stream;
    typedef hipEvent_t Event;
    static int stream_create(hipStream_t *s) { return (int)hipStreamCreateWithFlags(s, hipStreamNonBlocking); }
    static int event_create(hipEvent_t *e) { return (int)hipEventCreateWithFlags(e, hipEventDisableTiming); }
    static int timing_event_create(hipEvent_t *e) { return (int)hipEventCreate(e); }
    static void stream_destroy(hipStream_t s) { (void)hipStreamDestroy(s); }
    static void event_destroy(hipEvent_t e) { (void)hipEventDestroy(e); }
};
using namespace tfctx;             // CB_*, replace

struct tf_ctx {
    int device = 0, rank = 0, world = 1;
    mutable std::string err;
    // every device block of context lifetime, by name (tf_ctx_plan.h); the accessors below are their typed views
    tfscf::Blocks<CB_COUNT> blk{ctx_dev_alloc, ctx_dev_free};
    double *d_eri() const { return blk.at<double>(CB_ERI); }   // kept across builds (freeing and reallocating 27 GB costs ~1.4 s)
    double *scr(int k) const { return blk.at<double>(CB_SCR0 + k); }
    double *mo_pool() const { return blk.at<double>(CB_MO_POOL); }   // kept across calls
    double *d_jkstage() const { return blk.at<double>(CB_JKSTAGE); }
    double *d_agree() const { return blk.at<double>(CB_AGREE); }
    double *d_gtab() const { return blk.at<double>(CB_GTAB); }
    const int *d_csr_ptr() const { return blk.at<int>(CB_CSR_PTR); }
    const int *d_csr_idx() const { return blk.at<int>(CB_CSR_IDX); }
    const double *d_csr_val() const { return blk.at<double>(CB_CSR_VAL); }
    bool have_basis = false, have_eri = false;
    // the basis: committed together by tf_set_basis after its last upload, emptied together by free_basis
    tf::Basis bs;
    DBasis db{};                         // device copy of the basis (its blocks: basis_mem; lrec / tup: CB_LREC / CB_TUP, set by tf_build_eri)
    DeviceBlocks basis_mem;
    std::vector<DPair> host_pairs;      // host mirror of db.pairs (output offsets are filled in by tf_build_eri)
    DPair *d_pairs = nullptr;
    std::vector<int> pair_class;        // class id of every shell pair
    std::vector<int> h_ct_ix, h_ct_ord;  // host mirrors of DBasis::ct_ix / ct_ord / ct_sc (the team kernels' transform tables are built from them)
    std::vector<double> h_ct_sc;
    std::vector<std::vector<int>> class_pairs;   // pairs of each class, ascending
    // stored tensor
    int spherical = 1, N = 0, ld = 0;
    long long n_rows = 0;
    int2 *d_row_ij = nullptr;
    int *d_class_rows = nullptr, *d_row_pos = nullptr;   // packed layout: local rows listed class by class; position of a row in that order
    long long class_row_off[5] = {0, 0, 0, 0, 0};         // rows of class c: d_class_rows[class_row_off[c] .. class_row_off[c + 1])
    int *d_rowmap = nullptr;
    std::vector<int> my_pairs;          // bra shell pairs owned by this rank
    // packed (8-fold unique) layout: tf_jkpacked.hip.h
    int layout_req = -1;                // -1 auto, 0 rows (i >= j) x [k][l], 1 packed
    int layout = 0;
    long long n_elems = 0;              // stored doubles
    long long *d_rowoff = nullptr;
    int *d_rowsec = nullptr;            // [n_rows][6]: start of section a inside local row r; position in its storage unit, rows of the unit
    // parity-blocked layout tables (tf_layout.hip.h), host mirror (tf_packed_host.h) and device view
    tfp::HostLayout hl;
    BLayout bl{};
    // work tables of jk_packed_kernel: set 0 for one density per pass (groups of 8 rows), set 1 for two (groups of 4 rows)
    struct JKTables {
        JKGroup *d_groups = nullptr;
        JKTask *d_tasks = nullptr;
        JKSuper *d_supers = nullptr;
        int *d_gfirst = nullptr;        // [2][N]: first / one-past-last group with i == a
        int n_groups = 0, n_tasks = 0, n_supers = 0, nseg = 1;
        int bucket[4] = {0, 0, 0, 0};   // tasks [bucket[b], bucket[b + 1]) run with 4, 2, 1 waves per workgroup (b = 0, 1, 2)
        // the tasks a CLASS-DIAGONAL density needs (same order, same buckets): a row (i, j) of class c != 0 only meets P[j][l], P[j][k],
        // P[i][k], P[i][l] and the pair densities of class 0 -- every product of a task whose column class is neither i's nor j's is zero
        JKTask *d_tasks_cd = nullptr;
        int n_tasks_cd = 0, bucket_cd[4] = {0, 0, 0, 0};
        long long ypart_len = 0;
        JKJtPlan jp{};
    };
    // tiles layout (tf_tiles.h, tf_jktile.hip.h): host tables, their device copies and the partial-sum buffers of the Fock kernel
    tft::Tables tiles;
    tft::TaskList tsub1;                 // the one-density task list when its strips are shorter than the stored ones (TF_TILE_KSUB)
    int ksub1 = TT_KS;
    TView tv{};
    struct TileList {                    // device copy of a tft::TaskList + the partial-sum buffers of its passes
        TTask *d_tasks = nullptr;
        TPairI *d_pairs = nullptr;
        TRunI *d_runs = nullptr;
        int *d_itask_ptr = nullptr, *d_itasks = nullptr;
        int n_tasks = 0, bucket[TT_W + 1] = {0, 0, 0, 0, 0}, ksub = TT_KS, n_di = 0;
        long long dj_len = 0, jd_len = 0, jt_len = 0;
        double *DJ = nullptr, *Jt = nullptr, *Jd = nullptr, *DIk = nullptr, *DIl = nullptr;
        int nd_cap = 0;                  // densities the buffers are sized for
    };
    tft::TaskList tsubw;
    tft::ClassInfo tclass;               // what the list builder needs again for the wide list
    std::vector<std::pair<int, int>> trows;
    // The Fock state of a tensor build, grouped by layout (tf_jk_host.hip.h).  Every device block behind these pointers -- and behind the
    // tiles layout's view `tv` -- comes from build_mem and has the lifetime of the build: free_eri clears the owner and assigns a fresh
    // JkState, nothing is freed by name.
    struct JkAll {                       // every layout
        double *P = nullptr, *J = nullptr, *K = nullptr;   // the densities of one call of tf_fock_jk and their results
        double *Ppad = nullptr, *Jrow = nullptr;           // rows: padded densities; rows, packed: per-row Coulomb partials (zeroed once)
    };
    struct JkRows { double *Kp = nullptr; };
    struct JkPacked {
        JKTables t[2];
        int *jptr = nullptr;             // rows by second index x (internal): jrows[jptr[x] .. jptr[x + 1])
        int2 *jrows = nullptr;           // (local row, ORIGINAL first index of the row)
        int *xorder = nullptr;           // output rows of the exchange reduction, most partial vectors first
        JkPlan plan;                     // sizes, offsets and strides of the buffers below (tf_jk_plan.h)
        double *Psym = nullptr, *Pp = nullptr, *ypart = nullptr, *DI = nullptr, *DJ = nullptr, *Jt = nullptr, *D = nullptr;
        // second set of partial-sum buffers (JK_CD_JROW .. JK_CD_DJ) for passes over the class-diagonal task list (the entries its skipped
        // tasks would write stay zero, which the reductions rely on); allocated and zeroed at the first such pass
        double *cd[4] = {nullptr, nullptr, nullptr, nullptr};
        unsigned long long *cdflag = nullptr;   // device word: largest |P| between AOs of different classes (bit pattern)
    };
    struct JkTiles {
        TileList tl1, tlw;               // one density per pass (strips of ksub1 rows); 4 / 8 densities per pass (strips of 16 rows: built at first use)
        int *jlist_ptr = nullptr, *jlist = nullptr, *tvtab = nullptr;
        double *X = nullptr, *Pm = nullptr;   // [8][N][N] internal densities, [8] pair matrices
        double *out = nullptr;           // [6: Dj, Di, ED, EDT, JD, EJ][densities of the pass][N][N]; two such sets (the two passes of a general density)
        double *JtTot = nullptr;
    };
    struct JkState { JkAll all; JkRows rows; JkPacked packed; JkTiles tiles; } jk;
    DeviceBlocks build_mem;
    // (context lifetime: counters of tf_jk_path_stats; dynamic LDS limit requested for the tiles layout's edge / reduce kernels)
    long long jk_cd_passes = 0, jk_cd_declined = 0;
    size_t tile_lds_set = 48 * 1024;
    // instrumentation
    bool prof_jk = false;
    tfctx::EventPairs<HipHandles> prof;  // pairs (before, after) around the row kernel, on the launch stream
    void *comm = nullptr;                 // RCCL communicator of the ranks that share the tensor (tf_comm_init): the exchange step without a host callback
    tf_allreduce_fn allreduce = nullptr;  // completes partial [J;K] over the ranks of a sharded tensor (tf_set_allreduce)
    void *allreduce_user = nullptr;
    double eri_seconds[4] = {0, 0, 0, 0};
    long long eri_counts[3] = {0, 0, 0};
    long long eri_stats[TF_ERI_STAT_COUNT] = {};   // launches of the last build by kernel family (tf_eri_build_stats)
    double eri_nominal_flops = 0.0;      // the reference algorithm's operation count for the quartets of the last build
    tfscf::Workspace scf;
    std::vector<std::unique_ptr<tfscf::Workspace>> scf_batch;   // one workspace per cycle of a lockstep batch (tf_scf_rhf_batch), kept across calls
    tfdft::Grid grid;                    // Kohn-Sham integration grid with the AOs evaluated on it (tf_dft_setup)
    double xck_seconds[4] = {0, 0, 0, 0};   // the last exchange-correlation kernel build by stage (tf_xc_kernel_timings)
    int xck_spin_cols = 0;                   // column blocks per tile of the spin-blocked kernel build: 0 = XCK_SPIN_COLS (tf_xc_kernel_spin_cols)
    // persistent helpers of tf_build_eri (creating streams costs tens of ms per call); the J/K passes fork onto them while they are live
    tfctx::BuildStreams<HipHandles> bstr;
    static const int NSTREAM_MAX = tfctx::BuildStreams<HipHandles>::NSTREAM_MAX;
    size_t cfact_lds_set = 0;                // dynamic LDS limit requested for eri_cfact_kernel
    tfone::Arena arena1e;                    // device block for the short-lived buffers of the one-electron integrals
};

static int ensure_scratch(tf_ctx *ctx, int k, size_t bytes)
{
    const int e = ctx->blk.ensure(CB_SCR0 + k, bytes);
    if (e != 0) { ctx->err = std::string("hipMalloc of ERI scratch failed: ") + hipGetErrorString((hipError_t)e); return TF_ENOMEM; }
    return TF_OK;
}

#define TF_FAIL(ctx, code, ...)                                  \
    do {                                                         \
        char _b[512];                                            \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                   \
        (ctx)->err = _b;                                         \
        return (code);                                           \
    } while (0)

#define HIPCHK(ctx, call)                                                                          \
    do {                                                                                           \
        hipError_t _e = (call);                                                                    \
        if (_e != hipSuccess)                                                                      \
            TF_FAIL(ctx, (_e == hipErrorOutOfMemory ? TF_ENOMEM : TF_ENODEVICE), "%s failed: %s (%s:%d)", #call, \
                    hipGetErrorString(_e), __FILE__, __LINE__);                                    \
    } while (0)

// a host table into a new block that `owner` holds
template <class T>
static int upload(tf_ctx *ctx, const std::vector<T> &h, T **d, DeviceBlocks &owner)
{
    HIPCHK(ctx, owner.take((void **)d, std::max<size_t>(h.size(), 1) * sizeof(T)));
    if (!h.empty()) HIPCHK(ctx, hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return TF_OK;
}
// ... into a fresh block of the context's slot (the tables of context lifetime that change with every build)
template <class T>
static int upload(tf_ctx *ctx, const std::vector<T> &h, CtxBlock slot)
{
    HIPCHK(ctx, (hipError_t)replace(ctx->blk, slot, std::max<size_t>(h.size(), 1) * sizeof(T)));
    if (!h.empty()) HIPCHK(ctx, hipMemcpy(ctx->blk.p[slot], h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return TF_OK;
}

// out[q] = sum over the blocks, in block order, of d_part[block][q], q < k: the energies and
// integrals that are summed on the host (tf_corr_host.hip.h, tf_excited_host.hip.h, tf_dft_host.hip.h)
static hipError_t sum_partials_host(const double *d_part, int nblk, int k, double *out)
{
    std::vector<double> part((size_t)k * nblk);
    const hipError_t e = hipMemcpy(part.data(), d_part, part.size() * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    for (int q = 0; q < k; ++q) out[q] = 0.0;
    for (int b = 0; b < nblk; ++b)
        for (int q = 0; q < k; ++q) out[q] += part[(size_t)k * b + q];
    return hipSuccess;
}

// The blocks freed by free_eri / free_basis are recycled at once (tfcache): nothing queued earlier may still use them, hence the
// synchronisation.  If it FAILS the device is in an error state: the error is kept for the caller (tf_last_error), the cache is emptied
// and the blocks of this call go straight back to the runtime instead of being handed out again.
struct DrainedFree {
    bool ok;
    DrainedFree(tf_ctx *ctx, const char *what)
    {
        const hipError_t e = hipDeviceSynchronize();
        ok = e == hipSuccess;
        if (!ok) {
            ctx->err = std::string(what) + ": hipDeviceSynchronize failed before buffers were released (" + hipGetErrorString(e) + ")";
            tfcache::trim();
            tfcache::bypass = true;
        }
    }
    ~DrainedFree() { tfcache::bypass = false; }
};

static void free_eri(tf_ctx *ctx)
{
    DrainedFree drained(ctx, "free_eri");
    ctx->build_mem.clear();
    ctx->jk = tf_ctx::JkState();
    ctx->tv = TView{};
    ctx->bl = BLayout{};
    ctx->d_class_rows = ctx->d_row_pos = ctx->d_rowmap = ctx->d_rowsec = nullptr; ctx->d_row_ij = nullptr; ctx->d_rowoff = nullptr;
    ctx->n_elems = 0;
    ctx->have_eri = false;
}

static void free_basis(tf_ctx *ctx)
{
    DrainedFree drained(ctx, "free_basis");
    ctx->basis_mem.clear();
    for (int slot : {CB_CSR_PTR, CB_CSR_IDX, CB_CSR_VAL}) ctx->blk.drop(slot);
    // nothing that pointed into those blocks, or described the basis they held, survives them
    ctx->bs = tf::Basis();
    ctx->db = DBasis{};
    ctx->d_pairs = nullptr;
    ctx->host_pairs.clear(); ctx->pair_class.clear(); ctx->class_pairs.clear();
    ctx->h_ct_ix.clear(); ctx->h_ct_ord.clear(); ctx->h_ct_sc.clear();
    ctx->have_basis = false;
}
