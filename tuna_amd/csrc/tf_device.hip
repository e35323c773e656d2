// tf_device.hip -- context, device memory, launch logic and the C ABI of libtunafock.so (include/tunafock.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <array>
#include <cstring>
#include <condition_variable>
#include <dlfcn.h>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/tunafock.h"
#include "tf_internal.h"
#include "tf_kernels.hip.h"
#include "tf_jkpacked.hip.h"
#include "tf_packed_host.h"
#include "tf_tiles_host.h"
#include "tf_jk_plan.h"
#include "tf_jktile.hip.h"
#include "tf_eri.hip.h"
#include "tf_eri_team.hip.h"
#include "tf_eri_teamc.hip.h"
#include "tf_eri_team_api.h"
#include "tf_eri_plan.h"
#include "tf_oneel.hip.h"
#include "tf_scf.hip.h"
#include "tf_mp2.hip.h"
#include "tf_mp3.hip.h"
#include "tf_ccd.hip.h"
#include "tf_ccsd.hip.h"
#include "tf_cis.hip.h"
#include "tf_ucis.hip.h"
#include "tf_cisd.hip.h"
#include "tf_mp4.hip.h"
#include "tf_mp2dens.hip.h"
#include "tf_triples.hip.h"
#include "tf_dft.hip.h"
#include "tf_xckernel.hip.h"

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

struct tf_ctx {
    int device = 0, rank = 0, world = 1;
    mutable std::string err;
    tf::Basis bs;
    bool have_basis = false, have_eri = false;
    // device copy of the basis
    DBasis db{};
    std::vector<void *> basis_allocs;
    int *d_csr_ptr = nullptr, *d_csr_idx = nullptr;
    double *d_csr_val = nullptr;
    int csr_rows = 0;
    // stored tensor
    int spherical = 1, N = 0, ld = 0;
    long long n_rows = 0;
    double *d_eri = nullptr;
    size_t eri_cap = 0;                  // bytes allocated behind d_eri: kept across builds (freeing and reallocating 27 GB costs ~1.4 s)
    int2 *d_row_ij = nullptr;
    int *d_class_rows = nullptr, *d_row_pos = nullptr;   // packed layout: local rows listed class by class; position of a row in that order
    long long class_row_off[5] = {0, 0, 0, 0, 0};         // rows of class c: d_class_rows[class_row_off[c] .. class_row_off[c + 1])
    int *d_rowmap = nullptr;
    std::vector<int> my_pairs;          // bra shell pairs owned by this rank
    std::vector<DPair> host_pairs;      // host mirror of db.pairs (output offsets are filled in by tf_build_eri)
    DPair *d_pairs = nullptr;
    std::vector<int> pair_class;        // class id of every shell pair
    std::vector<int> h_ct_ix, h_ct_ord;  // host mirrors of DBasis::ct_ix / ct_ord / ct_sc (the team kernels' transform tables are built from them)
    std::vector<double> h_ct_sc;
    std::vector<std::vector<int>> class_pairs;   // pairs of each class, ascending
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
    std::vector<hipEvent_t> prof_ev;     // pairs (before, after) around the row kernel, on the launch stream
    size_t prof_used = 0;
    void *comm = nullptr;                 // RCCL communicator of the ranks that share the tensor (tf_comm_init): the exchange step without a host callback
    tf_allreduce_fn allreduce = nullptr;  // completes partial [J;K] over the ranks of a sharded tensor (tf_set_allreduce)
    void *allreduce_user = nullptr;
    double *d_jkstage = nullptr;          // [2][nd][N][N] staging buffer of that exchange step
    double *d_agree = nullptr;            // 16 doubles: per-iteration decision values summed over the ranks (agree_over_ranks)
    size_t jkstage_doubles = 0;
    double eri_seconds[4] = {0, 0, 0, 0};
    long long eri_counts[3] = {0, 0, 0};
    long long eri_stats[TF_ERI_STAT_COUNT] = {};   // launches of the last build by kernel family (tf_eri_build_stats)
    double eri_nominal_flops = 0.0;      // the reference algorithm's operation count for the quartets of the last build
    tfscf::Workspace scf;
    std::vector<std::unique_ptr<tfscf::Workspace>> scf_batch;   // one workspace per cycle of a lockstep batch (tf_scf_rhf_batch), kept across calls
    tfdft::Grid grid;                    // Kohn-Sham integration grid with the AOs evaluated on it (tf_dft_setup)
    double xck_seconds[4] = {0, 0, 0, 0};   // the last exchange-correlation kernel build by stage (tf_xc_kernel_timings)
    int xck_spin_cols = 0;                   // column blocks per tile of the spin-blocked kernel build: 0 = XCK_SPIN_COLS (tf_xc_kernel_spin_cols)
    // persistent helpers of tf_build_eri (creating streams / freeing GiB-sized buffers costs tens of ms per call)
    static const int NSTREAM_MAX = 8;
    hipStream_t streams[NSTREAM_MAX] = {};
    hipEvent_t sev[NSTREAM_MAX] = {};
    bool have_streams = false;
    hipStream_t cstream = nullptr;            // uploads of a slab's index lists (beside the kernels of the previous slab)
    hipEvent_t slab_done[2] = {nullptr, nullptr}, slab_lists[2] = {nullptr, nullptr};
    size_t cfact_lds_set = 0;                // dynamic LDS limit requested for eri_cfact_kernel
    tfk::LRec *d_lrec = nullptr;             // per-(La,Lb|Lc,Ld) records and entry index words of eri_cfact_kernel (per build)
    unsigned short *d_tup = nullptr;
    tfone::Arena arena1e;                    // device block for the short-lived buffers of the one-electron integrals
    double *d_gtab = nullptr;                // global-memory tables of the top angular momenta (eri_cfact_kernel<true, true>)
    size_t gtab_bytes = 0;
    double *scr[3] = {nullptr, nullptr, nullptr};
    size_t scr_bytes[3] = {0, 0, 0};
    double *mo_pool = nullptr;               // work space of the short-index-first AO->MO transformation (tfmp2::transform_q1), kept across calls
    size_t mo_pool_bytes = 0;
};

static int ensure_scratch(tf_ctx *ctx, int k, size_t bytes)
{
    if (bytes <= ctx->scr_bytes[k]) return TF_OK;
    if (ctx->scr[k]) { (void)tf_free(ctx->scr[k]); ctx->scr[k] = nullptr; ctx->scr_bytes[k] = 0; }
    hipError_t e = tf_malloc((void **)&ctx->scr[k], bytes);
    if (e != hipSuccess) { ctx->err = std::string("hipMalloc of ERI scratch failed: ") + hipGetErrorString(e); return TF_ENOMEM; }
    ctx->scr_bytes[k] = bytes;
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

template <class T>
static int upload(tf_ctx *ctx, const std::vector<T> &h, T **d, bool track = true)
{
    size_t bytes = std::max<size_t>(h.size(), 1) * sizeof(T);
    HIPCHK(ctx, tf_malloc((void **)d, bytes));
    if (track) ctx->basis_allocs.push_back(*d);
    if (!h.empty()) HIPCHK(ctx, hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return TF_OK;
}
// ... into a block that `owner` holds
template <class T>
static int upload(tf_ctx *ctx, const std::vector<T> &h, T **d, DeviceBlocks &owner)
{
    HIPCHK(ctx, owner.take((void **)d, std::max<size_t>(h.size(), 1) * sizeof(T)));
    if (!h.empty()) HIPCHK(ctx, hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
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

// ---- RCCL, loaded on demand (include/tunafock.h: tf_comm_*) ------------------------------------------------------------------------
namespace tfrccl {
typedef struct { char internal[128]; } UniqueId;                // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128)
typedef int (*GetUniqueId_t)(UniqueId *);
typedef int (*CommInitRank_t)(void **, int, UniqueId, int);
typedef int (*CommDestroy_t)(void *);
typedef int (*AllReduce_t)(const void *, void *, size_t, int, int, void *, hipStream_t);
typedef int (*Group_t)(void);
typedef const char *(*GetErrorString_t)(int);
static std::mutex mu;
static void *handle = nullptr;
static GetUniqueId_t GetUniqueId = nullptr;
static CommInitRank_t CommInitRank = nullptr;
static CommDestroy_t CommDestroy = nullptr;
static AllReduce_t AllReduce = nullptr;
static Group_t GroupStart = nullptr, GroupEnd = nullptr;
static GetErrorString_t GetErrorString = nullptr;
enum { kFloat64 = 8, kSum = 0 };                                   // ncclFloat64, ncclSum
static bool load(std::string &err)
{
    std::lock_guard<std::mutex> lk(mu);
    if (handle) return true;
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        handle = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (handle) break;
    }
    if (!handle) { err = std::string("librccl not found: ") + (dlerror() ? dlerror() : ""); return false; }
    GetUniqueId = (GetUniqueId_t)dlsym(handle, "ncclGetUniqueId"); CommInitRank = (CommInitRank_t)dlsym(handle, "ncclCommInitRank");
    CommDestroy = (CommDestroy_t)dlsym(handle, "ncclCommDestroy"); AllReduce = (AllReduce_t)dlsym(handle, "ncclAllReduce");
    GroupStart = (Group_t)dlsym(handle, "ncclGroupStart"); GroupEnd = (Group_t)dlsym(handle, "ncclGroupEnd");
    GetErrorString = (GetErrorString_t)dlsym(handle, "ncclGetErrorString");
    if (!GetUniqueId || !CommInitRank || !CommDestroy || !AllReduce || !GroupStart || !GroupEnd) { err = "librccl lacks an expected symbol"; dlclose(handle); handle = nullptr; return false; }
    return true;
}
static std::string errstr(int code) { return GetErrorString ? std::string(GetErrorString(code)) : ("code " + std::to_string(code)); }
}  // namespace tfrccl

// sum over the ranks of the attached communicator, in place, on stream st
static int comm_allreduce(tf_ctx *ctx, double *buf, size_t count, hipStream_t st)
{
    const int rc = tfrccl::AllReduce(buf, buf, count, tfrccl::kFloat64, tfrccl::kSum, ctx->comm, st);
    if (rc) TF_FAIL(ctx, TF_ENODEVICE, "ncclAllReduce failed: %s", tfrccl::errstr(rc).c_str());
    return TF_OK;
}

extern "C++" {
static int tile_list_upload(tf_ctx *ctx, const tft::TaskList &TL, bool own_shapes, tf_ctx::TileList &D);   // (tf_jk_host.hip.h; the tensor build uploads the first list)
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
    for (void *p : ctx->basis_allocs) (void)tf_free(p);
    ctx->basis_allocs.clear();
    for (void *p : {(void *)ctx->d_csr_ptr, (void *)ctx->d_csr_idx, (void *)ctx->d_csr_val})
        if (p) (void)tf_free(p);
    ctx->d_csr_ptr = ctx->d_csr_idx = nullptr; ctx->d_csr_val = nullptr;
    ctx->have_basis = false;
}

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

// Longest-processing-time assignment of row blocks (bra shell pairs) to ranks: heaviest block first, always to
// the least loaded rank.  Deterministic, so every rank computes the same plan without communication.
static void shard_plan(const std::vector<long long> &weight, int world, std::vector<int> &owner)
{
    const int n = (int)weight.size();
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return weight[x] > weight[y]; });
    std::vector<long long> load(world, 0);
    owner.assign(n, 0);
    for (int p : order) {
        const int r = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        load[r] += weight[p];
        owner[p] = r;
    }
}

// The plan of tf_build_eri (include/tunafock.h: tf_shard_plan_pairs).  Deterministic: every rank computes the same plan.
static void shard_plan_pairs(const std::vector<int> &dim, bool packed, int world, std::vector<int> &owner)
{
    const int ns = (int)dim.size();
    std::vector<long long> off(ns + 1, 0);
    for (int s = 0; s < ns; ++s) off[s + 1] = off[s] + dim[s];
    owner.assign((size_t)ns * (ns + 1) / 2, 0);
    std::vector<long long> load(world, 0);
    std::vector<long long> w;
    // WHOLE bra shells per rank when that balances (round 3): a rank then holds complete runs of j for its rows i -- super-groups as full
    // as on one GPU, and an eighth of the super-groups, so that the Jt partials and their reduction shrink with the shard.  (With every A
    // cut into `world` segments each rank keeps a short run of j under EVERY i: at N = 400 on 8 ranks the per-rank reduction stayed at
    // 0.08 ms -- as many super-groups per rank as on one GPU -- and the J/K kernel ran on one-group workgroups.)  Longest-processing-time
    // over the shells' weights; taken if the heaviest rank is within 3 % of the mean, else the segment plan below.  TF_SHARD_PLAN=segments
    // / shells forces one of the two (identically on every rank, of course).
    {
        const char *pe = getenv("TF_SHARD_PLAN");
        const bool force_seg = pe && pe[0] == 's' && pe[1] == 'e', force_sh = pe && pe[0] == 's' && pe[1] == 'h';
        if (world > 1 && !force_seg) {
            std::vector<long long> wA(ns, 0);
            long long total = 0;
            for (int A = 0; A < ns; ++A) {
                for (long long i = off[A]; i < off[A + 1]; ++i)
                    for (long long j = 0; j <= i; ++j) wA[A] += packed ? packed_row_len(i, j) : 1;
                total += wA[A];
            }
            std::vector<int> ord(ns);
            std::iota(ord.begin(), ord.end(), 0);
            std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return wA[x] > wA[y]; });
            std::vector<long long> ld(world, 0);
            std::vector<int> rankA(ns, 0);
            for (int A : ord) {
                const int r = (int)(std::min_element(ld.begin(), ld.end()) - ld.begin());
                ld[r] += wA[A];
                rankA[A] = r;
            }
            const long long heaviest = *std::max_element(ld.begin(), ld.end());
            if (force_sh || (double)heaviest * world <= 1.03 * (double)total) {
                for (int A = 0; A < ns; ++A)
                    for (int B = 0; B <= A; ++B) owner[(size_t)A * (A + 1) / 2 + B] = rankA[A];
                return;
            }
        }
    }
    for (int A = ns - 1; A >= 0; --A) {                           // heaviest rows first
        w.assign(A + 1, 0);
        long long total = 0;
        for (int B = 0; B <= A; ++B) {
            long long wb = 0;
            for (long long i = off[A]; i < off[A + 1]; ++i)
                for (long long j = off[B]; j < off[B + 1] && j <= i; ++j) wb += packed ? packed_row_len(i, j) : 1;
            w[B] = wb; total += wb;
        }
        // `world` contiguous segments of B with (nearly) equal weight
        struct Seg { int b0, b1; long long wt; };
        std::vector<Seg> segs;
        int b = 0;
        long long cum = 0;
        for (int sgi = 1; sgi <= world; ++sgi) {
            const long long target = (long long)((__int128)total * sgi / world);
            Seg sg{b, b, 0};
            while (b <= A && (sgi == world || cum + w[b] / 2 <= target)) { cum += w[b]; sg.wt += w[b]; ++b; }
            sg.b1 = b;
            segs.push_back(sg);
        }
        std::stable_sort(segs.begin(), segs.end(), [](const Seg &x, const Seg &y) { return x.wt > y.wt; });
        std::vector<int> ranks(world);
        std::iota(ranks.begin(), ranks.end(), 0);
        std::stable_sort(ranks.begin(), ranks.end(), [&](int x, int y) { return load[x] < load[y]; });
        for (int k = 0; k < world; ++k) {
            const Seg &sg = segs[k];
            for (int B = sg.b0; B < sg.b1; ++B) owner[(size_t)A * (A + 1) / 2 + B] = ranks[k];
            load[ranks[k]] += sg.wt;
        }
    }
}

extern "C" {

int tf_version(void) { return 100; }

int tf_shard_plan_pairs(int n_shells, const int32_t *dim, int layout, int world, int32_t *owner)
{
    if (n_shells < 0 || world < 1 || !dim || !owner || layout < 0 || layout > 1) return TF_EINVAL;
    std::vector<int> d(dim, dim + n_shells), o;
    shard_plan_pairs(d, layout >= 1, world, o);
    std::copy(o.begin(), o.end(), owner);
    return TF_OK;
}

int tf_shard_plan(int n_blocks, const int64_t *weight, int world, int32_t *owner)
{
    if (n_blocks < 0 || world < 1 || !weight || !owner) return TF_EINVAL;
    std::vector<long long> w(weight, weight + n_blocks);
    std::vector<int> o;
    shard_plan(w, world, o);
    std::copy(o.begin(), o.end(), owner);
    return TF_OK;
}

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
    if (ctx->d_eri) { (void)tf_free(ctx->d_eri); ctx->d_eri = nullptr; ctx->eri_cap = 0; }
    free_basis(ctx);
    tfscf::release(ctx->scf);
    for (auto &wsp : ctx->scf_batch) if (wsp) tfscf::release(*wsp);
    ctx->scf_batch.clear();
    tfdft::release(ctx->grid);
    for (hipEvent_t e : ctx->prof_ev) (void)hipEventDestroy(e);
    if (ctx->have_streams)
        for (int k = 0; k < tf_ctx::NSTREAM_MAX; ++k) { (void)hipStreamDestroy(ctx->streams[k]); (void)hipEventDestroy(ctx->sev[k]); }
    for (int k = 0; k < 3; ++k)
        if (ctx->scr[k]) (void)tf_free(ctx->scr[k]);
    if (ctx->mo_pool) (void)tf_free(ctx->mo_pool);
    if (ctx->comm) { (void)hipDeviceSynchronize(); (void)tfrccl::CommDestroy(ctx->comm); ctx->comm = nullptr; }
    if (ctx->d_jkstage) (void)tf_free(ctx->d_jkstage);
    if (ctx->d_agree) (void)tf_free(ctx->d_agree);
    if (ctx->d_lrec) (void)tf_free(ctx->d_lrec);
    if (ctx->d_tup) (void)tf_free(ctx->d_tup);
    if (ctx->d_gtab) (void)tf_free(ctx->d_gtab);
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
    std::string msg = tf::build_basis(ctx->bs, n_ao_cart, origin, lmn, prim_off, exps, coefs_raw);
    if (!msg.empty()) TF_FAIL(ctx, msg.find("aligned") != std::string::npos ? TF_EGEOM : TF_EINVAL, "%s", msg.c_str());
    const tf::Basis &bs = ctx->bs;
    std::vector<DShell> hs(bs.shells.size());
    for (size_t i = 0; i < hs.size(); ++i) hs[i] = {bs.shells[i].L, bs.shells[i].ncomp, bs.shells[i].comp_off, bs.shells[i].cart_off};
    std::vector<DPair> hp(bs.pairs.size());
    for (size_t i = 0; i < hp.size(); ++i) {
        const tf::Pair &p = bs.pairs[i];
        const tf::Shell &sa = bs.shells[p.A], &sb = bs.shells[p.B];
        hp[i] = {p.A, p.B, p.La, p.Lb, p.npp, p.pp_off, p.nE, 0, p.e_off, sa.ncomp, sb.ncomp, sa.comp_off, sb.comp_off, sa.cart_off, sb.cart_off, 0, 0};
    }
    // shell-pair classes: every pair of a class has the same angular momenta, component counts and contraction depth
    ctx->pair_class.assign(hp.size(), 0);
    ctx->class_pairs.clear();
    {
        // (shells that are not complete -- the one-component shells of the DECONTRACT ordering -- carry their components in the key: the
        // pairs of a class share one set of component-pair tables)
        auto comp_code = [&](const tf::Shell &sh) {
            if (sh.full) return 0;
            int code = 1;
            for (int c = 0; c < sh.ncomp && c < 2; ++c)
                code = code * 4096 + (bs.c_lx[sh.comp_off + c] | (bs.c_ly[sh.comp_off + c] << 4) | (bs.c_lz[sh.comp_off + c] << 8));
            return code;
        };
        std::map<std::array<int, 7>, int> ids;
        for (size_t i = 0; i < hp.size(); ++i) {
            const std::array<int, 7> key{hp[i].La, hp[i].Lb, getenv("TF_ERI_EXACT_CLASS") ? hp[i].npp : (hp[i].npp == 1 ? 1 : 0), hp[i].nca, hp[i].ncb,
                                         comp_code(bs.shells[bs.pairs[i].A]), comp_code(bs.shells[bs.pairs[i].B])};
            auto it = ids.find(key);
            if (it == ids.end()) { it = ids.emplace(key, (int)ids.size()).first; ctx->class_pairs.emplace_back(); }
            hp[i].cls = it->second;
            ctx->pair_class[i] = it->second;
            ctx->class_pairs[it->second].push_back((int)i);
        }
    }
    std::vector<double> boys;
    tf::boys_table(boys);
    DShell *d_sh; DPair *d_pr; int8_t *d_lx, *d_ly, *d_lz; double *d_sc, *d_p, *d_Pz, *d_K, *d_E, *d_boys;
    int rc;
    // per-L spherical rows as CSR over the Cartesian components of one shell
    std::vector<int> sph_base(TF_MAX_L + 2, 0), sph_ptr{0}, sph_idx;
    std::vector<double> sph_val;
    {
        std::vector<double> blk;
        for (int L = 0; L <= TF_MAX_L; ++L) {
            sph_base[L] = (int)sph_ptr.size() - 1;
            tf::sph_block(L, blk);
            const int nc = (L + 1) * (L + 2) / 2;
            for (int r = 0; r < 2 * L + 1; ++r) {
                for (int c = 0; c < nc; ++c)
                    if (blk[(size_t)r * nc + c] != 0.0) { sph_idx.push_back(c); sph_val.push_back(blk[(size_t)r * nc + c]); }
                sph_ptr.push_back((int)sph_idx.size());
            }
        }
    }
    // component-pair tables of every shell pair (eri_cfact_kernel): index word, normalisation ratio, position, parity-class order
    std::vector<int> ct_ix, ct_pos, ct_ord;
    std::vector<double> ct_sc;
    for (size_t i = 0; i < hp.size(); ++i) {
        DPair &pr = hp[i];
        const int nab = pr.nca * pr.ncb, L2 = pr.Lb + 1;
        pr.tab_off = (int)ct_ix.size();
        std::vector<int> cls(nab);
        for (int ca = 0; ca < pr.nca; ++ca)
            for (int cb = 0; cb < pr.ncb; ++cb) {
                const int a = pr.compoff_a + ca, b = pr.compoff_b + cb;
                const int ux = bs.c_lx[a], uy = bs.c_ly[a], uz = bs.c_lz[a], wx = bs.c_lx[b], wy = bs.c_ly[b], wz = bs.c_lz[b];
                const int c = ((ux + wx) & 1) | (((uy + wy) & 1) << 1);
                cls[ca * pr.ncb + cb] = c;
                ct_ix.push_back((ux * L2 + wx) | ((uy * L2 + wy) << 8) | ((uz * L2 + wz) << 16) | (c << 24));
                ct_pos.push_back((ca << 8) | cb);
                ct_sc.push_back(bs.c_scale[a] * bs.c_scale[b]);
            }
        pr.pcls[0] = 0;
        for (int c = 0; c < 4; ++c) {
            int n = 0;
            for (int f = 0; f < nab; ++f)
                if (cls[f] == c) { ct_ord.push_back(f); ++n; }
            pr.pcls[c + 1] = pr.pcls[c] + n;
        }
    }
    int *d_cti, *d_ctp, *d_cto; double *d_cts;
    if ((rc = upload(ctx, ct_ix, &d_cti)) || (rc = upload(ctx, ct_pos, &d_ctp)) || (rc = upload(ctx, ct_ord, &d_cto)) || (rc = upload(ctx, ct_sc, &d_cts)))
        return rc;
    int *d_sb, *d_sp, *d_si; double *d_sv;
    if ((rc = upload(ctx, hs, &d_sh)) || (rc = upload(ctx, hp, &d_pr)) || (rc = upload(ctx, bs.c_lx, &d_lx)) ||
        (rc = upload(ctx, bs.c_ly, &d_ly)) || (rc = upload(ctx, bs.c_lz, &d_lz)) || (rc = upload(ctx, bs.c_scale, &d_sc)) ||
        (rc = upload(ctx, bs.pp_p, &d_p)) || (rc = upload(ctx, bs.pp_Pz, &d_Pz)) || (rc = upload(ctx, bs.pp_K, &d_K)) ||
        (rc = upload(ctx, bs.epool, &d_E)) || (rc = upload(ctx, boys, &d_boys)) || (rc = upload(ctx, sph_base, &d_sb)) ||
        (rc = upload(ctx, sph_ptr, &d_sp)) || (rc = upload(ctx, sph_idx, &d_si)) || (rc = upload(ctx, sph_val, &d_sv)))
        return rc;
    ctx->db = DBasis{d_sh, d_pr, d_lx, d_ly, d_lz, d_sc, d_p, d_Pz, d_K, d_E, d_boys, d_sb, d_sp, d_si, d_sv, d_cti, d_ctp, d_cto, d_cts, nullptr, nullptr};
    ctx->host_pairs = hp;
    ctx->h_ct_ix = ct_ix; ctx->h_ct_ord = ct_ord; ctx->h_ct_sc = ct_sc;
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

// ---- the tensor build: uploads, struct EriBuild and its units, tf_build_eri, the tensor queries.  Included HERE,
// above the Fock build: the order in which the kernel templates are first used decides the order of the kernels in the code object.
#include "tf_eri_host.hip.h"

// ---- the Fock build: state of a tensor build, passes per layout, entry points.  Included HERE: the order in
// which the kernel templates are first used decides the order of the kernels in the code object, which stays what it was. -------------
#include "tf_jk_host.hip.h"
int EriBuild::alloc_jk_scratch() { return jk_alloc_state(ctx); }

// ---- collectives over the ranks, debug aids, the communicator ----------------------------------------------------------------------

// Collective control flow of the native cycles on a sharded tensor (tfscf::Workspace::agree): the values are summed over the ranks
// through the registered all-reduce; a rank whose values differ from the mean makes EVERY rank fail instead of leaving some of them
// waiting in the next collective.
static int agree_over_ranks(tf_ctx *ctx, const double *vals, int n, std::string &msg)
{
    if (ctx->world == 1 || (!ctx->allreduce && !ctx->comm)) return TF_OK;
    if (n > 7) n = 7;
    double h[16] = {0};
    h[0] = 1.0;
    for (int k = 0; k < n; ++k) { h[1 + k] = vals[k]; h[8 + k] = vals[k] * vals[k]; }
    if (!ctx->d_agree && tf_malloc((void **)&ctx->d_agree, 16 * sizeof(double)) != hipSuccess) { msg = "hipMalloc failed (agree buffer)"; return TF_ENOMEM; }
    if (hipMemcpy(ctx->d_agree, h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess) { msg = "hipMemcpy failed (agree buffer)"; return TF_ENODEVICE; }
    int rc;
    if (ctx->comm) { rc = comm_allreduce(ctx, ctx->d_agree, 16, nullptr); if (rc) { msg = ctx->err; return rc; } }
    else rc = ctx->allreduce(ctx->allreduce_user, ctx->d_agree, 16, nullptr);
    if (rc) { msg = "the registered all-reduce failed (code " + std::to_string(rc) + ")"; return TF_ENODEVICE; }
    double s[16];
    if (hipMemcpy(s, ctx->d_agree, sizeof(s), hipMemcpyDeviceToHost) != hipSuccess) { msg = "hipMemcpy failed (agree buffer)"; return TF_ENODEVICE; }
    // slot 15 is the status word of the hook's convention (distributed.py: a rank whose staging failed adds 1 to the last element)
    if (s[15] != 0.0) { msg = "the exchange of the agreement vector failed on at least one rank"; return TF_ENODEVICE; }
    const double w = (double)ctx->world;
    bool same = s[0] == w;
    // all equal <=> sum of squares == (sum)^2 / world (small integers and flags: exact in double precision)
    for (int k = 0; k < n && same; ++k) same = (s[1 + k] == w * vals[k]) && (s[8 + k] == w * vals[k] * vals[k]);
    if (!same) {
        msg = "the ranks of the sharded SCF cycle disagree on a control decision (convergence / DIIS history / step): every rank stops";
        return TF_ELINALG;
    }
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

int tf_set_allreduce(tf_ctx *ctx, tf_allreduce_fn fn, void *user)
{
    if (!ctx) return TF_EINVAL;
    ctx->allreduce = fn; ctx->allreduce_user = user;
    return TF_OK;
}

int tf_comm_unique_id(void *id_out)
{
    if (!id_out) return TF_EINVAL;
    std::string err;
    if (!tfrccl::load(err)) { g_create_error = err; return TF_ENODEVICE; }
    tfrccl::UniqueId id;
    const int rc = tfrccl::GetUniqueId(&id);
    if (rc) { g_create_error = "ncclGetUniqueId failed: " + tfrccl::errstr(rc); return TF_ENODEVICE; }
    std::memcpy(id_out, &id, sizeof(id));
    return TF_OK;
}

int tf_comm_init(tf_ctx *ctx, const void *id, int comm_rank, int comm_size)
{
    if (!ctx || !id || comm_size < 1 || comm_rank < 0 || comm_rank >= comm_size) return TF_EINVAL;
    std::string err;
    if (!tfrccl::load(err)) TF_FAIL(ctx, TF_ENODEVICE, "%s", err.c_str());
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->comm) { (void)tfrccl::CommDestroy(ctx->comm); ctx->comm = nullptr; }
    tfrccl::UniqueId uid;
    std::memcpy(&uid, id, sizeof(uid));
    void *comm = nullptr;
    const int rc = tfrccl::CommInitRank(&comm, comm_size, uid, comm_rank);
    if (rc) TF_FAIL(ctx, TF_ENODEVICE, "ncclCommInitRank failed: %s", tfrccl::errstr(rc).c_str());
    ctx->comm = comm;
    return TF_OK;
}

int tf_comm_destroy(tf_ctx *ctx)
{
    if (!ctx) return TF_EINVAL;
    if (ctx->comm) {
        (void)hipSetDevice(ctx->device);
        (void)hipDeviceSynchronize();
        (void)tfrccl::CommDestroy(ctx->comm);
        ctx->comm = nullptr;
    }
    return TF_OK;
}

int tf_comm_attached(const tf_ctx *ctx) { return (ctx && ctx->comm) ? 1 : 0; }

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

// ---- SCF --------------------------------------------------------------------------------------------

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

// ---- Kohn-Sham exchange-correlation (next row of the hot path: SURVEY.md section 8f rank 2) --------------------------

#include "tf_dft_host.hip.h"

// ---- AO->MO transformation, MP2 ... CCSD(T), the MP2 density: the drivers of the correlated methods (consumers of the resident tensor) ----
#include "tf_corr_host.hip.h"
// ---- CIS / TDHF, TD-DFT / TDA, the stability analysis, CIS(D): the drivers of the excited states, on the shared pieces of the above ----
#include "tf_excited_host.hip.h"

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
    if (!ctx) return TF_EINVAL;
    if (!ctx->have_eri) TF_FAIL(ctx, TF_EINVAL, "tf_scf_uhf: call tf_build_eri first");
    if (!opts || !S || !T || !V || !P0_alpha || !P0_beta || !out || n_alpha < 1 || n_alpha > ctx->N || n_beta < 0 || n_beta > n_alpha)
        TF_FAIL(ctx, TF_EINVAL, "tf_scf_uhf: bad arguments");
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
    if (!ctx) return TF_EINVAL;
    if (!ctx->have_eri) TF_FAIL(ctx, TF_EINVAL, "tf_scf_uks: call tf_build_eri first");
    if (!opts || !S || !T || !V || !P0_alpha || !P0_beta || !out || n_alpha < 1 || n_alpha > ctx->N || n_beta < 0 || n_beta > n_alpha)
        TF_FAIL(ctx, TF_EINVAL, "tf_scf_uks: bad arguments");
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

}  // extern "C"
