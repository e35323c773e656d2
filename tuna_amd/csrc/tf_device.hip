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
    for (void *p : {(void *)ctx->d_csr_ptr, (void *)ctx->d_csr_idx, (void *)ctx->d_csr_val})
        if (p) (void)tf_free(p);
    int rc;
    if ((rc = upload(ctx, ptr, &ctx->d_csr_ptr, false)) || (rc = upload(ctx, idx, &ctx->d_csr_idx, false)) ||
        (rc = upload(ctx, val, &ctx->d_csr_val, false)))
        return rc;
    ctx->csr_rows = (int)ptr.size() - 1;
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
// ---- the tensor build: tf_build_eri is a short sequence of units over one plan -----------------------------
// The device lists and timing events that live for ONE build.  release() is what the end of a successful build does (the device is
// drained by then); the destructor covers every other way out: launches may still be in flight, so it drains the device first.
struct EriBuildMem {
    tf_ctx *ctx;
    std::vector<void *> blocks;
    std::vector<hipEvent_t> events;
    explicit EriBuildMem(tf_ctx *c) : ctx(c) {}
    EriBuildMem(const EriBuildMem &) = delete;
    template <class T> int alloc(T **p, size_t bytes)
    {
        HIPCHK(ctx, tf_malloc((void **)p, bytes));
        blocks.push_back(*p);
        return TF_OK;
    }
    template <class T> int up(const std::vector<T> &h, T **d)
    {
        *d = nullptr;
        const int rc = upload(ctx, h, d, false);
        if (*d) blocks.push_back(*d);
        return rc;
    }
    void drop(void *p)                                              // a list that is replaced by a larger one
    {
        if (!p) return;
        blocks.erase(std::remove(blocks.begin(), blocks.end(), p), blocks.end());
        (void)tf_free(p);
    }
    int event(hipEvent_t *e)
    {
        HIPCHK(ctx, hipEventCreate(e));
        events.push_back(*e);
        return TF_OK;
    }
    void release()
    {
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        for (void *p : blocks) (void)tf_free(p);
        events.clear(); blocks.clear();
        ctx->db.kq_ptr = ctx->db.kq_off = ctx->db.kt_ptr = ctx->db.kt_k = nullptr; ctx->db.kt_c = nullptr;
    }
    ~EriBuildMem()
    {
        if (blocks.empty() && events.empty()) return;
        (void)hipDeviceSynchronize();
        release();
    }
};

// The plan of one build: what the units below share.  plan_storage and plan_generation fill it, run_slab walks it.
struct EriBuild {
    tf_ctx *ctx;
    const tf::Basis &bs;
    const tfp::HostLayout &H;
    const int spherical;
    EriBuildMem mem;
    EriBuild(tf_ctx *c, int sph) : ctx(c), bs(c->bs), H(c->hl), spherical(sph), mem(c) {}

    // storage
    int Nc = 0, N = 0, ld = 0, npairs = 0, nsh = 0, ncls = 0;
    bool packed = false, tiles = false;
    long long row_len = 0;
    std::vector<long long> pair_rows;
    std::vector<int> owner;
    tfp::RowTables rows;
    // slab size, work counters
    bool per_class = false;
    double *d_C = nullptr, *d_T2 = nullptr;
    long long max_rows_c = 1, cut_rows = 1;                     // rows the slab buffers hold; rows at which run_slab cuts (<= max_rows_c)
    double t_stage[4] = {0, 0, 0, 0};
    long long n_quart = 0, n_primq = 0, n_compq = 0;
    std::vector<long long> cum_pairs, cum_pp, cum_comp;
    std::vector<std::array<double, 4>> pairW, pairNc, cumW;
    std::vector<std::array<double, 44>> cumNL;
    double nominal_flops = 0.0;
    std::chrono::steady_clock::time_point t_wall0;
    // ket lists, groups and families
    static constexpr int NLPG = 7, NGRP = 2 * NLPG;
    static constexpr int FAM_MM = 9, FAM_MA_CC = 3;
    std::vector<int> ket_sorted, ket_off, cls_maxnpp;
    int kets_goff[NGRP + 1] = {};
    int *d_kets = nullptr, *d_kets_all = nullptr;
    std::vector<int> kets_all_host;                              // same order as d_kets_all
    bool fam_off = false, cc_fam_off = false, bra_fam_on = false, fam_any = false;
    std::vector<int> fam_heads, fam_ptr{0}, fam_mem;
    int fam_goff[NGRP + 1] = {};
    int *d_fam_heads = nullptr, *d_fam_ptr = nullptr, *d_fam_mem = nullptr;
    std::vector<int> psid;
    std::vector<int> mine_sorted;
    // streams
    int NSTREAM = 1;
    hipStream_t *streams = nullptr;
    hipEvent_t *sev = nullptr;
    int launch_count = 0;
    long long stats[TF_ERI_STAT_COUNT] = {};                   // host counters of tf_eri_build_stats: incremented where the launches are made
    void count(int family) { ++stats[family]; ++stats[TF_ERI_STAT_LAUNCHES]; }
    // launch tables
    std::vector<LRec> lrecs_host;                              // per (La, Lb | Lc, Ld), filled by make_lrecs
    hipError_t team_error = hipSuccess;                        // first failed launch of a team kernel
    bool use_team_pc = false, use_teamc = false, use_team = false;
    int teamc_pqmax = 700;
    struct KClassTab { int pS[5] = {0, 0, 0, 0, 0}; int nkap = 0, nnzT = 0, tp_off = 0, te_off = 0; };
    std::vector<KClassTab> kct;
    int *d_kq_ptr = nullptr, *d_kq_off = nullptr, *d_kt_ptr = nullptr, *d_kt_k = nullptr, *d_kcnt = nullptr;
    double *d_kt_c = nullptr;
    KetRec *d_ketrec = nullptr;                                // parallel to d_kets (class-sorted ket list)
    int *d_tflat = nullptr;                                    // flat component / output lists of the class pairs (TClass::flat_off)
    std::vector<int> flat_off;
    BraRec *d_brarec = nullptr;                                // parallel to the slab's bra list d_bra
    const int *d_bra_base = nullptr;
    struct GroupStat { int maxLp = 0, maxT = 1, maxLp1 = 1, maxE = 0, maxcomp = 1, maxnpp = 1; };
    CFCaps gcaps[NGRP][NGRP];
    bool gcaps_fit[NGRP][NGRP], gcaps_gtab[NGRP][NGRP];
    struct BraFam { int *d_ptr = nullptr, *d_mem = nullptr; unsigned n = 0; };
    typedef std::map<std::pair<size_t, int>, BraFam> BraFams;  // by (first position of the run of bra pairs, largest family)
    // the slabs' index lists (two sets) and timing events
    size_t cap_bra = 0, cap_out = 0, out_bytes = 0, rowcls_bytes = 0;
    int *d_bra = nullptr, *d_bra_alloc = nullptr;
    long long *d_braoff = nullptr, *d_braoff_alloc = nullptr;
    void *d_out = nullptr, *d_out_alloc = nullptr;
    BraRec *d_brarec_alloc = nullptr;
    signed char *d_rowcls = nullptr, *d_rowcls_alloc = nullptr;  // parity class of every slab row (small-problem mode, packed layout)
    long long slab_no = 0;
    std::vector<hipEvent_t> tev;                                   // 4 timing events per slab, read at the end
    std::vector<hipEvent_t> tev2;                                  // 2 per slab around the task-list team kernels (they count as ERI kernels)
    size_t cursor = 0;
    // small-problem mode with team kernels
    std::vector<TClass> tcs_host;
    std::vector<int> tc_of, tc_team;                               // -2: not made yet, -1: not eligible
    std::vector<size_t> tc_lds;
    bool any_wide_pair = false;                                    // a pair sum beyond the team kernels' instantiations
    int max_npp_all = 1;
    TClass *d_tcs = nullptr; TeamTask *d_tasks = nullptr;
    size_t d_tcs_cap = 0, d_tasks_cap = 0;
    struct TcLaunch { int LAB, LCD, team; size_t lds; std::vector<TeamTask> tasks; std::vector<double> cost; };

    int out_dim(const tf::Shell &s) const { return spherical ? s.nsph : s.ncomp; }
    int out_off(const tf::Shell &s) const { return spherical ? s.sph_off : s.cart_off; }
    long long pair_cost(int p) const {                             // primitive pairs x components: what a quartet with this pair costs
        return (long long)bs.pairs[p].npp * bs.shells[bs.pairs[p].A].ncomp * bs.shells[bs.pairs[p].B].ncomp;
    }
    // groups of shell pairs: by La + Lb (0-1, 2-3, 4-5, 6-7, 8, 9, 10: the table sizes grow with the fourth power of L, and only the
    // very top -- (hh|hh), (hh|gh), ... -- exceeds LDS and falls back to the component-per-lane kernel) and by contracted / uncontracted
    static int lp_group(int lp) { return lp <= 1 ? 0 : (lp <= 3 ? 1 : (lp <= 5 ? 2 : (lp <= 7 ? 3 : std::min(lp - 4, 6)))); }
    int pair_group(int p) const { return 2 * lp_group(bs.pairs[p].La + bs.pairs[p].Lb) + (bs.pairs[p].npp > 1 ? 1 : 0); }

    int plan_storage();
    int upload_consumer_tables();
    int plan_generation();
    int plan_slab_size();
    void plan_work_counters();
    int plan_ket_lists();
    int plan_ket_families();
    int setup_streams();
    int plan_team_tables();
    int plan_index_buffers();
    TClass tclass_common(int bcls, int kcls, int &maxblk, int &maxK, int &nnzc) const;
    void launch_class(int bcls, int kcls, int max_npp_bra, unsigned n_bra, const int *d_bra, const long long *d_braoff, int bra_Amax);
    void launch_generic_old(unsigned n_bra, const int *d_bra, const long long *d_braoff, unsigned n_ket, const int *d_ket, hipStream_t st);
    GroupStat group_stat(const int *pairs_host, size_t n) const;
    void make_caps();
    int make_lrecs(bool with_caps);
    const BraFam *bra_families(BraFams &bra_fams, const std::vector<int> &bra_host, size_t b0, size_t b1, int most);
    int launch_generic(const std::vector<int> &bra_host, const int *d_bra, const long long *d_braoff);
    int teamc_class(int bcls, int kcls);
    int teamc_tasks(const std::vector<int> &bra, const std::vector<long long> &braoff, std::vector<TcLaunch> &tcl, bool &old_needed);
    int launch_teamc(const std::vector<TcLaunch> &tcl);
    int run_slab();
    int finish();
    int alloc_jk_scratch();
};

// Storage: layout choice, owners of the bra shell pairs, host tables (tf_packed_host.h / tf_tiles_host.h), tensor buffer, table uploads
int EriBuild::plan_storage()
{
    int rc;
    Nc = bs.n_cart; N = spherical ? bs.n_sph : bs.n_cart; ld = (N + 1) & ~1;
    if (ctx->grid.G > 0 && ctx->grid.N != N) tfdft::release(ctx->grid);   // (a grid of the other AO representation)
    ctx->spherical = spherical; ctx->N = N; ctx->ld = ld;
    npairs = (int)bs.pairs.size();

    // ---- which bra shell pairs (= row blocks) belong to this rank: longest-processing-time on row counts
    for (int p = 0; p < npairs; ++p) {
        ctx->host_pairs[p].outoff_a = out_off(bs.shells[bs.pairs[p].A]);
        ctx->host_pairs[p].outoff_b = out_off(bs.shells[bs.pairs[p].B]);
    }
    HIPCHK(ctx, hipMemcpy(ctx->d_pairs, ctx->host_pairs.data(), (size_t)npairs * sizeof(DPair), hipMemcpyHostToDevice));
    // layout: packed (8-fold unique, tf_jkpacked.hip.h) unless asked otherwise
    int layout = ctx->layout_req;
    if (const char *e = getenv("TF_ERI_LAYOUT")) layout = (e[0] == 't') ? 2 : ((e[0] == 'p') ? 1 : (e[0] == 'r' ? 0 : layout));
    if (layout < 0) layout = 1;                                       // (tiles: opt-in -- measured slower than packed at N = 400)
    ctx->layout = layout;
    // packed: the symmetry-unique, parity-allowed values (layouts 1 and 2: the generation and its slab are the same); tiles: stored
    // j-innermost in (i, class pair, strip, chunk) regions (tf_tiles.h) instead of row by row (tf_jkpacked.hip.h)
    packed = layout >= 1; tiles = layout == 2;
    pair_rows.assign(npairs, 0);
    for (int p = 0; p < npairs; ++p) {
        const tf::Shell &a = bs.shells[bs.pairs[p].A], &b = bs.shells[bs.pairs[p].B];
        pair_rows[p] = (bs.pairs[p].A == bs.pairs[p].B) ? (long long)out_dim(a) * (out_dim(a) + 1) / 2
                                                        : (long long)out_dim(a) * out_dim(b);
    }
    {
        std::vector<int> dims(bs.shells.size());
        for (size_t q = 0; q < dims.size(); ++q) dims[q] = out_dim(bs.shells[q]);
        shard_plan_pairs(dims, packed, ctx->world, owner);           // pair index A(A+1)/2 + B = position in bs.pairs
    }
    ctx->my_pairs.clear();
    for (int p = 0; p < npairs; ++p)
        if (owner[p] == ctx->rank) ctx->my_pairs.push_back(p);

    // ---- parity classes of the output AOs and the layout tables (packed layout)
    if (packed) {
        std::vector<int> cls;
        tfp::ao_classes(bs, spherical != 0, cls);
        if ((rc = build_blocked_layout(ctx, cls))) return rc;
    }
    // ---- row tables
    {
        std::vector<int> ooff(bs.shells.size()), odim(bs.shells.size());
        for (size_t q = 0; q < odim.size(); ++q) { ooff[q] = out_off(bs.shells[q]); odim[q] = out_dim(bs.shells[q]); }
        tfp::list_rows(bs.pairs, ooff, odim, ctx->my_pairs, N, rows);
    }
    if (packed) tfp::pack_rows(H, tiles, rows);
    const std::vector<TFInt2> &row_ij = rows.row_ij;
    if (packed && !tiles) ctx->n_elems = rows.n_elems;
    if (tiles) {
        // regions of the stored tensor and the task list of the Fock kernel (tf_tiles_host.h)
        const tft::ClassInfo C = tfp::class_info(H);
        std::vector<std::pair<int, int>> rows_ij(row_ij.size());
        for (size_t r = 0; r < row_ij.size(); ++r) rows_ij[r] = {H.sigma[row_ij[r].x], H.sigma[row_ij[r].y]};
        static const int part_steps = std::min(TT_STEPS_MAX, getenv("TF_TILE_PART_STEPS") ? std::max(1, atoi(getenv("TF_TILE_PART_STEPS"))) : TT_STEPS_MAX);
        ctx->tclass = C; ctx->trows = rows_ij;
        std::string e = tft::build(C, rows_ij, part_steps, ctx->tiles);
        if (!e.empty()) TF_FAIL(ctx, TF_EINVAL, "%s", e.c_str());
        static const int ksub_env = getenv("TF_TILE_KSUB") ? atoi(getenv("TF_TILE_KSUB")) : 32;     // (measured at N = 400: strips of 32 rows 2.2 ms, of 64 3.0, of 16 2.3)
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
        V.regions = d_regions; V.prim_pairs = d_pp; V.prim_runs = d_rr; V.edge_base = TT.edge_base; V.N = N; V.pm_len = TT.pm_len; V.tab = Z.tvtab;
        ctx->tv = V;
        Z.tl1.d_pairs = d_pp; Z.tl1.d_runs = d_rr;
    }
    ctx->n_rows = (long long)row_ij.size();
    row_len = (long long)N * ld;
    if (!packed) ctx->n_elems = ctx->n_rows * row_len;
    if (ctx->n_rows > 0x7fffffffLL) TF_FAIL(ctx, TF_EINVAL, "too many tensor rows for this build");
    {
        // the tensor buffer is kept across builds (geometry scans rebuild a tensor of the same size); it is replaced when it is
        // too small or more than twice too large
#ifdef TF_ABL_ALLVALID
        const size_t need = std::max<size_t>(1, (size_t)ctx->n_elems * sizeof(double)) + (4u << 20);
#else
        const size_t need = std::max<size_t>(1, (size_t)ctx->n_elems * sizeof(double));
#endif
        if (ctx->d_eri && (ctx->eri_cap < need || ctx->eri_cap > 2 * need + (64u << 20))) {
            (void)tf_free(ctx->d_eri);
            ctx->d_eri = nullptr; ctx->eri_cap = 0;
        }
        if (!ctx->d_eri) {
            HIPCHK(ctx, tf_malloc((void **)&ctx->d_eri, need));
            ctx->eri_cap = need;
        }
    }
    if ((rc = upload_int2(ctx, row_ij, &ctx->d_row_ij)) || (rc = upload(ctx, rows.rowmap, &ctx->d_rowmap, ctx->build_mem))) return rc;
    if (packed) {
        if (!tiles && ((rc = upload(ctx, rows.rowoff, &ctx->d_rowoff, ctx->build_mem)) || (rc = upload(ctx, rows.rowsec, &ctx->d_rowsec, ctx->build_mem)))) return rc;
        ctx->db.bl = ctx->bl;
        ctx->db.RLS = H.RLS;
    }
    if (tiles) HIPCHK(ctx, hipMemsetAsync(ctx->d_eri, 0, (size_t)ctx->n_elems * sizeof(double), 0));   // the pad slots of the rows and pieces stay zero
    return TF_OK;
}

// The tables only the CONSUMERS of the tensor need (work tables of the J/K kernel, reduction lists, rows by class) are built on the
// host while the generation kernels run: called behind the launches of the last slab (7 ms of host time at N = 400).
int EriBuild::upload_consumer_tables()
{
    if (!packed) return TF_OK;
    int rc2;
    tfp::ConsumerTables CT;
    tfp::build_class_rows(H, rows, CT);
    std::copy(CT.class_row_off, CT.class_row_off + 5, ctx->class_row_off);
    DeviceBlocks &mem = ctx->build_mem;
    if ((rc2 = upload(ctx, CT.class_rows, &ctx->d_class_rows, mem)) || (rc2 = upload(ctx, CT.row_pos, &ctx->d_row_pos, mem))) return rc2;
    if (tiles) {
        const tft::Tables &TT = ctx->tiles;
        const tft::TaskList &TL = ctx->ksub1 == TT_KS ? TT.primary : ctx->tsub1;
        tf_ctx::JkTiles &Z = ctx->jk.tiles;
        if ((rc2 = tile_list_upload(ctx, TL, ctx->ksub1 != TT_KS, Z.tl1)) || (rc2 = upload(ctx, TT.jlist_ptr, &Z.jlist_ptr, mem)) ||
            (rc2 = upload(ctx, TT.jlist, &Z.jlist, mem)))
            return rc2;
        return TF_OK;
    }
    tf_ctx::JkPacked &K = ctx->jk.packed;
    if ((rc2 = upload_jk_tables(ctx, rows, JKShape<1>::RB, K.t[0])) || (rc2 = upload_jk_tables(ctx, rows, JKShape<2>::RB, K.t[1]))) return rc2;
    tfp::build_reduction_lists(H, rows, CT);
    if ((rc2 = upload(ctx, CT.jptr, &K.jptr, mem)) || (rc2 = upload_int2(ctx, CT.jrows, &K.jrows))) return rc2;
    if ((rc2 = upload(ctx, CT.xorder, &K.xorder, mem))) return rc2;
    return TF_OK;
}

// ---- slabs of bra pairs: Cartesian block -> ket transform -> bra transform -> tensor rows
int EriBuild::plan_slab_size()
{
    int rc;
    // Large problems launch per (bra class, ket class) with the ket transform fused into the ERI kernels: no Cartesian slab at all.
    per_class = (long long)ctx->my_pairs.size() * npairs >= 2000000LL;
    if (const char *m = getenv("TF_ERI_MODE")) per_class = (m[0] == 'c');
    // A slab row is one Cartesian bra component pair: Nc^2 Cartesian ket values (small-problem mode only) and the ket-transformed
    // row -- N x ld (rows layout) or the complete-row shape of the packed layout (RLS doubles, ~ N^2 / 8).  1 GiB of slab, more (up
    // to 4 GiB) for big tensors: fewer, larger class launches.
    const size_t cart_row_bytes = (size_t)Nc * Nc * sizeof(double);
    const size_t t2_row_bytes = (packed ? (size_t)H.RLS : (size_t)N * ld) * sizeof(double);
    const size_t slab_row_bytes = std::max<size_t>(8, std::max(t2_row_bytes, per_class ? (size_t)0 : cart_row_bytes));
    size_t slab_total = 0;                                       // this rank's bra rows: one slab if that is <= 4 GiB
    for (int p : ctx->my_pairs) slab_total += (size_t)bs.shells[bs.pairs[p].A].ncomp * bs.shells[bs.pairs[p].B].ncomp * slab_row_bytes;
    size_t slab_bytes = std::min<size_t>((size_t)4 << 30, std::max<size_t>((size_t)1 << 30, std::max((size_t)ctx->n_elems, slab_total)));
    if (const char *e = getenv("TF_SLAB_MB")) slab_bytes = (size_t)std::max(1, atoi(e)) << 20;
    max_rows_c = std::max<long long>(1, (long long)(slab_bytes / slab_row_bytes));
    // TF_SLAB_ROWS=n: the slab in Cartesian bra rows (the 1 MiB floor of TF_SLAB_MB cannot cut a small basis); n = 1 gives one bra
    // shell pair per slab, the finest cut there is
    cut_rows = 0;
    if (const char *e = getenv("TF_SLAB_ROWS")) max_rows_c = cut_rows = std::max<long long>(1, atoll(e));
    long long biggest = 1;
    for (int p : ctx->my_pairs)
        biggest = std::max<long long>(biggest, (long long)bs.shells[bs.pairs[p].A].ncomp * bs.shells[bs.pairs[p].B].ncomp);
    max_rows_c = std::max(max_rows_c, biggest);
    {
        long long need = 0;                                      // never more than this rank's rows need
        for (int p : ctx->my_pairs) need += (long long)bs.shells[bs.pairs[p].A].ncomp * bs.shells[bs.pairs[p].B].ncomp;
        max_rows_c = std::max<long long>(biggest, std::min(max_rows_c, need));
    }
    // the buffers hold the largest pair; the cut itself stays at what TF_SLAB_ROWS asked for (a slab always takes its first pair whole)
    cut_rows = cut_rows ? std::min(cut_rows, max_rows_c) : max_rows_c;
    if ((rc = ensure_scratch(ctx, 0, per_class ? 8 : (size_t)max_rows_c * cart_row_bytes)) ||
        (rc = ensure_scratch(ctx, 2, (size_t)max_rows_c * t2_row_bytes)))
        return rc;
    d_C = ctx->scr[0]; d_T2 = ctx->scr[2];
    return TF_OK;
}

void EriBuild::plan_work_counters()
{
    // work counters: ket pairs / primitive pairs / component pairs with first shell <= A (the pair list is A-major).  The packed
    // layout computes exactly the kets whose first shell does not exceed the bra's; the rows layout all of them.
    nsh = (int)bs.shells.size();
    cum_pairs.assign(nsh + 1, 0); cum_pp.assign(nsh + 1, 0); cum_comp.assign(nsh + 1, 0);
    for (int p = 0; p < npairs; ++p) {
        const int A = bs.pairs[p].A;
        cum_pairs[A + 1] += 1;
        cum_pp[A + 1] += bs.pairs[p].npp;
        cum_comp[A + 1] += (long long)bs.shells[A].ncomp * bs.shells[bs.pairs[p].B].ncomp;
    }
    for (int a = 0; a < nsh; ++a) { cum_pairs[a + 1] += cum_pairs[a]; cum_pp[a + 1] += cum_pp[a]; cum_comp[a + 1] += cum_comp[a]; }
    // Nominal operation count of the reference algorithm for the quartets this build evaluates: per primitive
    // AO quartet that passes the parity test (pyx:1324-1327), 8 x the inner terms of the loop nest pyx:1179-1217 -- (lx12/2+1)(lx34/2+1)
    // (ly12/2+1)(ly34/2+1)(lz12+1)(lz34+1), a product of a bra and a ket factor -- plus the Boys / R table cost 6 (L+1) + 3 (L+1)^2 / 2 + 60.
    // Per shell pair and parity class c: W = sum of its factor over the component pairs of the class, n = their number.
    pairW.resize(npairs); pairNc.resize(npairs);
    for (int p = 0; p < npairs; ++p) {
        const tf::Shell &sa = bs.shells[bs.pairs[p].A], &sb = bs.shells[bs.pairs[p].B];
        pairW[p] = {0, 0, 0, 0}; pairNc[p] = {0, 0, 0, 0};
        for (int ca = 0; ca < sa.ncomp; ++ca)
            for (int cb = 0; cb < sb.ncomp; ++cb) {
                const int u = sa.comp_off + ca, v = sb.comp_off + cb;
                const int lx = bs.c_lx[u] + bs.c_lx[v], ly = bs.c_ly[u] + bs.c_ly[v], lz = bs.c_lz[u] + bs.c_lz[v];
                const int c = (lx & 1) | ((ly & 1) << 1);
                pairW[p][c] += (double)((lx / 2 + 1) * (ly / 2 + 1) * (lz + 1));
                pairNc[p][c] += 1.0;
            }
    }
    // prefix sums over the first shell A of the ket pairs (the pair list is A-major): npp x W per class, and npp x n per class and Lc + Ld
    cumW.assign(nsh + 1, std::array<double, 4>{0, 0, 0, 0});
    cumNL.resize(nsh + 1);
    for (auto &x : cumNL) x.fill(0.0);
    for (int p = 0; p < npairs; ++p) {
        const int A = bs.pairs[p].A, lcd = std::min(10, bs.pairs[p].La + bs.pairs[p].Lb);
        for (int c = 0; c < 4; ++c) {
            cumW[A + 1][c] += (double)bs.pairs[p].npp * pairW[p][c];
            cumNL[A + 1][4 * lcd + c] += (double)bs.pairs[p].npp * pairNc[p][c];
        }
    }
    for (int a = 0; a < nsh; ++a) {
        for (int c = 0; c < 4; ++c) cumW[a + 1][c] += cumW[a][c];
        for (int x = 0; x < 44; ++x) cumNL[a + 1][x] += cumNL[a][x];
    }
}

int EriBuild::plan_ket_lists()
{
    int rc;
    // class-sorted ket lists on the device (one contiguous range per class)
    ncls = (int)ctx->class_pairs.size();
    ket_off.assign(ncls + 1, 0); cls_maxnpp.assign(ncls, 1);
    for (int c = 0; c < ncls; ++c) {
        ket_sorted.insert(ket_sorted.end(), ctx->class_pairs[c].begin(), ctx->class_pairs[c].end());
        ket_off[c + 1] = (int)ket_sorted.size();
        for (int p : ctx->class_pairs[c]) cls_maxnpp[c] = std::max(cls_maxnpp[c], bs.pairs[p].npp);
    }
    if ((rc = mem.up(ket_sorted, &d_kets))) return rc;
    {
        // generic (single-launch) mode: heaviest ket pairs first -- workgroups are dispatched in index order, and a deeply contracted
        // (pp|pp) quartet of Ar2/cc-pVQZ runs for 12 ms: it has to start early, not at the tail of the launch
        // the launches are made per (bra group, ket group) of shell pairs -- groups by La + Lb -- so that the LDS carve-out of each
        // launch fits its own angular momenta (the (gg|gg) tables need 100 KB, the (ss|ss) ones nothing)
        std::vector<int> all(npairs);
        std::iota(all.begin(), all.end(), 0);
        std::stable_sort(all.begin(), all.end(), [&](int x, int y) {
            const int gx = pair_group(x), gy = pair_group(y);
            return gx != gy ? gx < gy : pair_cost(x) > pair_cost(y);
        });
        for (int p : all) ++kets_goff[pair_group(p) + 1];
        for (int g = 0; g < NGRP; ++g) kets_goff[g + 1] += kets_goff[g];
        if ((rc = mem.up(all, &d_kets_all))) return rc;
        kets_all_host = all;
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
    const double prim_quartets_est = 0.5 * (double)cum_pp[nsh] * (double)cum_pp[nsh];
    fam_off = getenv("TF_ERI_FAMILIES") ? getenv("TF_ERI_FAMILIES")[0] == '0' : prim_quartets_est < 8.0e6;
    cc_fam_off = getenv("TF_ERI_CC_FAMILIES") && getenv("TF_ERI_CC_FAMILIES")[0] == '0';
    bra_fam_on = !fam_off && getenv("TF_ERI_BRA_FAMILIES") && getenv("TF_ERI_BRA_FAMILIES")[0] == '1';
    psid.assign(bs.shells.size(), -1);
    {
        int nid = 0;
        for (size_t a = 0; a < bs.shells.size(); ++a) {
            if (psid[a] >= 0) continue;
            psid[a] = nid;
            const tf::Shell &sa = bs.shells[a];
            for (size_t b = a + 1; b < bs.shells.size(); ++b) {
                const tf::Shell &sb = bs.shells[b];
                if (psid[b] >= 0 || sb.z != sa.z || sb.L != sa.L || sb.nprim != sa.nprim || sb.ncomp != sa.ncomp || sb.full != sa.full) continue;
                bool same = true;
                for (int q = 0; q < sa.nprim && same; ++q) same = bs.s_exp[sa.prim_off + q] == bs.s_exp[sb.prim_off + q];
                for (int q = 0; q < sa.ncomp && same; ++q)
                    same = bs.c_lx[sa.comp_off + q] == bs.c_lx[sb.comp_off + q] && bs.c_ly[sa.comp_off + q] == bs.c_ly[sb.comp_off + q] &&
                           bs.c_lz[sa.comp_off + q] == bs.c_lz[sb.comp_off + q] && bs.c_scale[sa.comp_off + q] == bs.c_scale[sb.comp_off + q];
                if (same) psid[b] = nid;
            }
            ++nid;
        }
        for (int g = 0; g < NGRP; ++g) {
            fam_goff[g] = (int)fam_heads.size();
            if (!(g & 1) || fam_off) continue;                     // contracted groups only
            std::map<std::pair<int, int>, std::vector<int>> open_fam;   // key -> index of the family still taking members (in fam_ptr order)
            std::vector<std::vector<int>> fams;
            for (int k = kets_goff[g]; k < kets_goff[g + 1]; ++k) {
                const int p = kets_all_host[k];
                const auto key = std::make_pair(psid[bs.pairs[p].A], psid[bs.pairs[p].B]);
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
                if (f.size() > 1) fam_any = true;
            }
        }
        fam_goff[NGRP] = (int)fam_heads.size();
        if (fam_any) {
            if ((rc = mem.up(fam_heads, &d_fam_heads)) || (rc = mem.up(fam_ptr, &d_fam_ptr)) ||
                (rc = mem.up(fam_mem, &d_fam_mem)))
                return rc;
        }
    }
    return TF_OK;
}

// streams so that the many small class launches of a slab overlap
int EriBuild::setup_streams()
{
    const int NSTREAM_MAX = tf_ctx::NSTREAM_MAX;
    NSTREAM = getenv("TF_ERI_NSTREAM") ? std::max(1, std::min(NSTREAM_MAX, atoi(getenv("TF_ERI_NSTREAM")))) : NSTREAM_MAX;
    if (!ctx->have_streams) {
        for (int k = 0; k < NSTREAM_MAX; ++k) {
            HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->streams[k], hipStreamNonBlocking));
            HIPCHK(ctx, hipEventCreateWithFlags(&ctx->sev[k], hipEventDisableTiming));
        }
        HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->cstream, hipStreamNonBlocking));
        for (auto &e : ctx->slab_done) HIPCHK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (auto &e : ctx->slab_lists) HIPCHK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->have_streams = true;
    }
    streams = ctx->streams;
    sev = ctx->sev;
    return TF_OK;
}

// the class-wide part of a team kernel's class record (tf_eri_team.hip.h) for (bra pair class, ket pair class)
TClass EriBuild::tclass_common(int bcls, int kcls, int &maxblk, int &maxK, int &nnzc) const
{
    const DPair &hb = ctx->host_pairs[ctx->class_pairs[bcls][0]], &hk = ctx->host_pairs[ctx->class_pairs[kcls][0]];
    const KClassTab &kt = kct[kcls];
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
    q.npp_ab = max_npp_bra; q.npp_cd = cls_maxnpp[kcls]; q.npq = q.npp_ab * q.npp_cd;      // class maxima (LDS sizing)
    q.nEab = pb.nE; q.nEcd = pk.nE;
    q.n_ket = ket_off[kcls + 1] - ket_off[kcls];
    if (packed) {
        const std::vector<int> &kl = ctx->class_pairs[kcls];
        q.n_ket = (int)(std::upper_bound(kl.begin(), kl.end(), bra_Amax, [&](int a, int p) { return a < bs.pairs[p].A; }) - kl.begin());
        if (q.n_ket == 0) return;
    }
    q.fused = 1; q.spherical = spherical ? 1 : 0;
    q.nsc = spherical ? sc.nsph : sc.ncomp; q.nsd = spherical ? sd.nsph : sd.ncomp;
    q.Nout = N; q.ld = ld;
    q.tri = packed ? 1 : 0;
    double *d_out_slab = d_T2;                               // fused kernels write the half-transformed slab directly
    const int *d_ket = d_kets + ket_off[kcls];
    hipStream_t st = streams[launch_count++ % NSTREAM];
    // TF_ERI_CLASS_TIMES=1 (diagnostic): every class launch alone on the device, its time printed with the class
    static const bool class_times = getenv("TF_ERI_CLASS_TIMES") != nullptr;
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
    } class_timer(class_times, q, n_bra);
    if (use_team_pc && q.npq == 1 && q.La + q.Lb <= TF_TEAM_LMAX && q.Lc + q.Ld <= TF_TEAM_LMAX) {
        // one shell quartet per team of lanes, tables private to the team (tf_eri_team.hip.h)
        int maxblk = 1, maxK = 1, nnzc = 0;
        TClass t = tclass_common(bcls, kcls, maxblk, maxK, nnzc);
        t.n_ket = q.n_ket;
        const int LAB = q.La + q.Lb, LCD = q.Lc + q.Ld, NM = q.L / 2 + 1, XS = NM | 1, RSr = q.L + 2;
        auto even = [](int x) { return (x + 1) & ~1; };
        int o = 0;
        t.oE12 = o; o += even(2 * t.nEab);
        t.oOffA = o; o += 2 * t.nab;
        t.oScA = o; o += even(t.nab);
        t.oOffK = o; o += 2 * t.ncd;
        t.oTp = o; o += even((t.nkap + 2) / 2);
        t.oTk = o; o += even((t.nnzT + 1) / 2);
        t.oTc = o; o += even(t.nnzT);
        t.oRowOff = o; o += t.nab;
        const int foff = flat_off.empty() ? -1 : flat_off[(size_t)bcls * ncls + kcls];
        auto vmax_of = [](int tm) { return tm == 256 ? 2048 : (tm == 64 ? 512 : 96); };
        const int nacc_pad = even(nnzc);
        t.oCompW = o; t.oOutW = o + nacc_pad / 2; t.flat_off = std::max(0, foff); t.nflat = nacc_pad + 2 * t.nout;
        const int flat_doubles = even((t.nflat + 1) / 2);
        const int shared_noflat = o;
        t.shared_doubles = o;
        const int nG = t.nTcd * (LAB + 1) * NM, scr1 = 2 * t.nEcd + (q.L + 1) * RSr + nG;
        // (a class whose parity-allowed components fit the team's block runs the flat lists: one loop over all components)
        auto flat_for = [&](int tm) { return foff >= 0 && nnzc <= vmax_of(tm); };
        auto vcap_of = [&](int tm) { return flat_for(tm) ? even(std::max(scr1, nnzc)) : even(std::max(scr1, std::max(maxK, std::min(maxblk, vmax_of(tm))))); };
        auto team_doubles_of = [&](int tm) { return 2 * t.nT * XS + vcap_of(tm) + even((t.nkap + 1) / 2); };
        auto bytes_of = [&](int tm) { return ((size_t)shared_noflat + (flat_for(tm) ? flat_doubles : 0) + (size_t)(256 / tm) * team_doubles_of(tm)) * sizeof(double); };
        // lanes per quartet: 16 for the smallest classes; a wave while four quartets' tables fit about half of the LDS (two workgroups per
        // CU); the whole workgroup beyond.  (Measured at N = 400, ERI kernels: 36 / 52 / 76 / 100 KB limit: 35.3 / 32.8 / 31.9 / 33 ms.)
        static const int force_team = getenv("TF_ERI_TEAM_SIZE") ? atoi(getenv("TF_ERI_TEAM_SIZE")) : 0;
        static const int lds_kb = getenv("TF_TEAM_LDS_KB") ? atoi(getenv("TF_TEAM_LDS_KB")) : 76;
        static const int t16_nnz = getenv("TF_TEAM16_NNZ") ? atoi(getenv("TF_TEAM16_NNZ")) : 96;
        static const long long kpw_div = getenv("TF_TEAM_KPW_DIV") ? atoll(getenv("TF_TEAM_KPW_DIV")) : 2048;
        static const long long kpw_max = getenv("TF_TEAM_KPW_MAX") ? atoll(getenv("TF_TEAM_KPW_MAX")) : 16;
        int team = 0;
        if (t.nT <= 16 && nnzc <= t16_nnz && eri_team_available(LAB, LCD, 16)) team = 16;
        else if (eri_team_available(LAB, LCD, 64) && bytes_of(64) <= (size_t)lds_kb * 1024) team = 64;
        else if (eri_team_available(LAB, LCD, 256) && bytes_of(256) <= 160 * 1024 - 256) team = 256;
        else if (eri_team_available(LAB, LCD, 64) && bytes_of(64) <= 160 * 1024 - 256) team = 64;
        if (force_team && eri_team_available(LAB, LCD, force_team) && bytes_of(force_team) <= 160 * 1024 - 256) team = force_team;
        if (team) {
            const int NT = 256 / team;
            t.vcap = vcap_of(team); t.team_doubles = team_doubles_of(team);
            t.flat = flat_for(team) ? 1 : 0;
            t.shared_doubles = shared_noflat + (t.flat ? flat_doubles : 0);
            // a workgroup walks over several ket groups (shared staging once): enough workgroups to fill the chip, at most 16 groups each
            // (measured at N = 400, ERI kernels: >= 65536 / 16384 / 4096 / 2048 / 1024 / 512 workgroups per launch aimed at:
            // 36.0 / 32.8 / 28.3 / 26.8 / 26.5-27.1 / 27.9 ms)
            const long long groups = (q.n_ket + NT - 1) / NT;
            const long long kpw = std::max<long long>(1, std::min<long long>(kpw_max, groups * n_bra / kpw_div));
            TeamLaunch a{LAB, LCD, team, dim3((unsigned)((groups + kpw - 1) / kpw), n_bra), bytes_of(team), st, &ctx->db, &t,
                         d_brarec + (d_bra - d_bra_base), d_ketrec + ket_off[kcls], d_kcnt + (size_t)kcls * nsh, d_out_slab};
            const hipError_t e = eri_team_launch(a);
            if (e != hipSuccess) { team_error = e; }
            count(team == 16 ? TF_ERI_STAT_TEAM16 : (team == 64 ? TF_ERI_STAT_TEAM64 : TF_ERI_STAT_TEAM256));
            if (t.flat) ++stats[TF_ERI_STAT_TEAM_FLAT];
            return;
        }
    }
    if (q.npq == 1 && q.ncomp <= 128) {
        // several uncontracted shell quartets per workgroup
        int ncp = 1;
        while (ncp < q.ncomp) ncp <<= 1;
        q.ncp = ncp;
        q.G = std::max(1, std::min(TF_ERI_THREADS / ncp, TF_ERI_THREADS / (q.L + 1)));
        q.PB = q.G; q.stride = q.G | 1;
        const int kc = q.ncc + q.ncd;
        int o = 0;
        q.offR = o; o += q.stride * q.tsize;
        q.offPref = o; o += q.G;
        q.offPQ = o; o += q.G;
        q.offRed = o;
        q.offEab = o; o += 2 * q.nEab;
        q.offEcd = o; o += q.G * 2 * q.nEcd;
        q.offScale = o; o += 42 + kc * q.G;
        q.offLmn = o; o += (42 + kc * q.G + q.G + 1) / 2;
        q.offBlk = o; o += q.G * q.ncomp;
        q.offCsr = o; o += TF_CSR_DOUBLES;
        q.lds_doubles = o;
        const dim3 grid((q.n_ket + q.G - 1) / q.G, n_bra);
        count(TF_ERI_STAT_MULTI);
        hipLaunchKernelGGL(eri_multi_kernel, grid, dim3(TF_ERI_THREADS), (size_t)o * sizeof(double), st, ctx->db, q, d_bra, d_braoff,
                           d_ket, Nc, d_out_slab);
    } else if (q.npq == 1 && (q.La + 1) * (q.Lb + 1) * (q.Lc + 1) * (q.Ld + 1) * 2 * (q.L / 2 + 1) <= 7000 && !getenv("TF_ERI_NOFACT")) {
        // uncontracted, many components: per-axis factor tables in LDS
        const int nT = (q.La + 1) * (q.Lb + 1) * (q.Lc + 1) * (q.Ld + 1), nM = q.L / 2 + 1;
        q.PB = 1; q.stride = 1; q.G = 1; q.ncp = 0;
        const LRec &lr = lrecs_host[((q.La * 6 + q.Lb) * 6 + q.Lc) * 6 + q.Ld];
        q.tupG_off = lr.tupG_off; q.tupXZ_off = lr.tupXZ_off;
        int o = 0;
        q.offR = o; o += q.tsize;
        q.offPref = o; o += 2;
        q.offPQ = o; o += 2;
        q.offEab = o; o += 2 * q.nEab;
        q.offEcd = o; o += 2 * q.nEcd;
        const int tables_end = o;                            // R, prefactors and E tables: dead once X and Z are built
        q.offScale = o; o += 84;
        q.offLmn = o; o += 42;
        q.offRed = o; o += 2 * nT * nM;                      // X and Z tables
        const int nG = (q.Lc + 1) * (q.Ld + 1) * (q.La + q.Lb + 1) * nM;
        q.offBlk = o; o += std::max((int)TF_BLK_DOUBLES, nG);   // the ket half of the z tables lives here until the components start
        q.offG = q.offBlk;
        q.offTab = o; o += 2 * (q.nca * q.ncb + q.ncc * q.ncd) + 2;
        if (tables_end >= TF_CSR_DOUBLES) q.offCsr = 0;      // staged over the dead tables (after the X/Z barrier)
        else { q.offCsr = o; o += TF_CSR_DOUBLES; }
        q.lds_doubles = o;
        // (TF_ERI_FACT_THREADS=64|128: smaller workgroups for experiments -- measured slower at N = 400, 127 / 159 ms against 113-127 ms:
        // the LDS of a quartet limits the workgroups per CU, so fewer waves per workgroup are fewer waves per CU)
        static const int force_thr = getenv("TF_ERI_FACT_THREADS") ? atoi(getenv("TF_ERI_FACT_THREADS")) : 0;
        const int fact_threads = (force_thr == 64 || force_thr == 128) ? force_thr : TF_ERI_THREADS;
        count(TF_ERI_STAT_FACT);
        hipLaunchKernelGGL(eri_fact_kernel, dim3(q.n_ket, n_bra), dim3(fact_threads), (size_t)o * sizeof(double), st, ctx->db, q, d_bra,
                           d_braoff, d_ket, Nc, d_out_slab);
    } else {
        const int RB = 3584, EB = 3072;                     // LDS doubles for R tables / staged E tables
        int PB = RB / q.tsize - 1;
        PB = std::max(1, std::min(std::min(PB, TF_ERI_THREADS), q.npq));
        q.PB = PB; q.stride = PB | 1; q.G = 1; q.ncp = 0;
        const int needE = q.npp_ab * 2 * q.nEab + q.npp_cd * 2 * q.nEcd;
        const bool stage = needE <= EB;
        int o = 0;
        q.offR = o; o += q.stride * q.tsize;
        q.offPref = o; o += TF_ERI_THREADS;
        q.offPQ = o; o += TF_ERI_THREADS;
        q.offRed = o; o += TF_ERI_THREADS;
        q.offEab = o; o += stage ? q.npp_ab * 2 * q.nEab : 0;
        q.offEcd = o; o += stage ? q.npp_cd * 2 * q.nEcd : 0;
        q.offScale = o; o += 84;
        q.offLmn = o; o += 42;
        q.offBlk = o; o += TF_BLK_DOUBLES;
        q.offCsr = o; o += TF_CSR_DOUBLES;
        q.lds_doubles = o;
        const dim3 grid(q.n_ket, n_bra);
        count(stage ? TF_ERI_STAT_CLASS_STAGED : TF_ERI_STAT_CLASS_UNSTAGED);
        if (stage)
            hipLaunchKernelGGL((eri_class_kernel<true, false>), grid, dim3(TF_ERI_THREADS), (size_t)o * sizeof(double), st, ctx->db, q,
                               d_bra, d_braoff, d_ket, Nc, d_out_slab);
        else
            hipLaunchKernelGGL((eri_class_kernel<false, false>), grid, dim3(TF_ERI_THREADS), (size_t)o * sizeof(double), st, ctx->db, q,
                               d_bra, d_braoff, d_ket, Nc, d_out_slab);
    }
}

// Small problems: per slab one launch per (bra group, ket group), each mixing the classes of its groups (LDS carved by the
// capacities the groups need).  bra_host: the slab's bra pairs (sorted by group).
void EriBuild::launch_generic_old(unsigned n_bra, const int *d_bra, const long long *d_braoff, unsigned n_ket, const int *d_ket, hipStream_t st)
{
    QClass q{};
    const int RB = 2048, EBa = 1024, EBc = 1024;       // (doubling the E capacities halves the occupancy: Ar2 build 0.084 -> 0.18 s)
    int o = 0;
    q.offR = o; o += RB;
    q.offPref = o; o += TF_ERI_THREADS;
    q.offPQ = o; o += TF_ERI_THREADS;
    q.offRed = o; o += TF_ERI_THREADS;
    q.offEab = o; o += EBa;
    q.offEcd = o; o += EBc;
    q.offScale = o; o += 84;
    q.offLmn = o; o += 42;
    q.lds_doubles = o;
    q.offBlk = o;                                            // unused (unfused)
    q.G = 1; q.n_ket = (int)n_ket; q.fused = 0;
    q.tri = packed ? 1 : 0;
    count(TF_ERI_STAT_COMPONENT_LANE);
    hipLaunchKernelGGL((eri_class_kernel<true, true>), dim3(n_ket, n_bra), dim3(TF_ERI_THREADS), (size_t)o * sizeof(double), st,
                       ctx->db, q, d_bra, d_braoff, d_ket, Nc, d_C);
}

EriBuild::GroupStat EriBuild::group_stat(const int *pairs_host, size_t n) const
{
    GroupStat g;
    for (size_t k = 0; k < n; ++k) {
        const tf::Pair &pr = bs.pairs[pairs_host[k]];
        g.maxLp = std::max(g.maxLp, pr.La + pr.Lb);
        g.maxT = std::max(g.maxT, (pr.La + 1) * (pr.Lb + 1));
        g.maxE = std::max(g.maxE, pr.npp * 2 * pr.nE);
        g.maxcomp = std::max(g.maxcomp, bs.shells[pr.A].ncomp * bs.shells[pr.B].ncomp);
        g.maxnpp = std::max(g.maxnpp, pr.npp);
    }
    g.maxLp1 = g.maxLp + 1;
    return g;
}

// LDS carve-out of the launch (bra group gb, ket group gk), from the largest angular momenta / contraction depths of the groups
void EriBuild::make_caps()
{
    GroupStat gs[NGRP];
    for (int g = 0; g < NGRP; ++g) gs[g] = group_stat(kets_all_host.data() + kets_goff[g], (size_t)(kets_goff[g + 1] - kets_goff[g]));
    for (int gb = 0; gb < NGRP; ++gb)
        for (int gk = 0; gk < NGRP; ++gk) {
            const GroupStat &sb = gs[gb], &sk = gs[gk];
            const int Lmax = sb.maxLp + sk.maxLp, nM = Lmax / 2 + 1, tsize = (Lmax + 1) * (Lmax + 2) / 2;
            const int xz = sb.maxT * sk.maxT * nM, gsz = sk.maxT * sb.maxLp1 * nM;
            const bool deep = sb.maxnpp > 1 || sk.maxnpp > 1;
            // batch size aimed at and LDS doubles for the X / Z tables and the staged Hermite tables (tuning knobs; smaller carve-outs
            // mean more workgroups per CU: Ar2/cc-pVQZ ERI kernels 21.1 ms with 48 / 1536 / 1536, 18.3 ms with 24 / 768 / 1024)
            static const int k_nbt = getenv("TF_CF_NBT") ? atoi(getenv("TF_CF_NBT")) : 24, k_xz = getenv("TF_CF_XZ") ? atoi(getenv("TF_CF_XZ")) : 768;
            static const int k_e = getenv("TF_CF_E") ? atoi(getenv("TF_CF_E")) : 1024;
            const int nbt = deep ? std::min(TF_ERI_THREADS / (Lmax + 1), k_nbt) : 1;       // primitive quartets per batch aimed at
            CFCaps c{};
            int o = 0;
            c.offR = o; c.capR = std::max(2 * tsize, std::min((nbt + 1) * tsize, 2 * k_xz * 2 / 3)); o += c.capR;
            c.offPref = o; o += TF_ERI_THREADS;
            c.offPQ = o; o += TF_ERI_THREADS;
            c.offPP = o; o += TF_ERI_THREADS;
            c.offG = o; c.capG = std::max(gsz, std::min(nbt * gsz, k_xz * 2 / 3)); o += c.capG;
            c.capXZ = std::max(xz, std::min(nbt * xz, k_xz));
            c.offX = o; o += c.capXZ;
            c.offZ = o; o += c.capXZ;
            c.offTupG = o; o += (gsz + 3) / 4;
            c.offTupXZ = o; o += (xz + 3) / 4;
            c.offEab = o; c.capEab = std::min(sb.maxE, k_e); o += c.capEab;
            c.offEcd = o; c.capEcd = std::min(sk.maxE, k_e); o += c.capEcd;
            c.offRed = o; o += TF_ERI_THREADS;
            c.offKm = o; c.capKm = fam_off ? 0 : FAM_MM * (((gk & 1) ? sk.maxnpp : 0) + ((gb & 1) ? sb.maxnpp : 0)); o += c.capKm;
            c.lds_doubles = o;
            c.tri = packed ? 1 : 0;
            c.dbg_npq_lo = 0; c.dbg_npq_hi = 0x7fffffff;
            c.team_lmax = use_teamc ? TF_TEAM_LMAX : -1; c.team_pqmax = teamc_pqmax;
            if (const char *e = getenv("TF_ERI_DBG_NPQ")) (void)sscanf(e, "%d:%d", &c.dbg_npq_lo, &c.dbg_npq_hi);
            gcaps[gb][gk] = c;
            gcaps_fit[gb][gk] = (size_t)o * sizeof(double) <= 160 * 1024 - 256;
            gcaps_gtab[gb][gk] = false;
            if (!gcaps_fit[gb][gk] && !deep) {
                // (hh|hh)-sized tables: G, X and Z of a workgroup go to global memory, everything else stays in LDS
                CFCaps d = c;
                int q = 0;
                d.offR = q; q += d.capR;
                d.offPref = q; q += TF_ERI_THREADS;
                d.offPQ = q; q += TF_ERI_THREADS;
                d.offPP = q; q += TF_ERI_THREADS;
                d.offTupG = q; q += (gsz + 3) / 4;
                d.offTupXZ = q; q += (xz + 3) / 4;
                d.offEab = q; q += d.capEab;
                d.offEcd = q; q += d.capEcd;
                d.offRed = q; q += TF_ERI_THREADS;
                d.offKm = q; q += d.capKm;
                d.lds_doubles = q;
                d.capG = gsz; d.capXZ = xz;
                d.offG = 0; d.offX = gsz; d.offZ = gsz + xz;
                d.gtab_doubles = gsz + 2 * xz;
                if ((size_t)q * sizeof(double) <= 160 * 1024 - 256) { gcaps[gb][gk] = d; gcaps_fit[gb][gk] = true; gcaps_gtab[gb][gk] = true; }
            }
        }
}

// per (La, Lb | Lc, Ld): table sizes, index words of the table entries, batch capacity under the caps of its launch
int EriBuild::make_lrecs(bool with_caps)
{
    std::vector<LRec> recs(6 * 6 * 6 * 6, LRec{});
    std::vector<unsigned short> tup;
    std::vector<char> seen_pair(36, 0);
    for (const tf::Pair &pr : bs.pairs) seen_pair[pr.La * 6 + pr.Lb] = 1;
    auto grp_of = [&](int lp) { return lp_group(lp); };
    for (int ab = 0; ab < 36; ++ab)
        for (int cd = 0; cd < 36; ++cd) {
            if (!seen_pair[ab] || !seen_pair[cd]) continue;
            const int La = ab / 6, Lb = ab % 6, Lc = cd / 6, Ld = cd % 6;
            const int gb = grp_of(La + Lb), gk = grp_of(Lc + Ld);
            LRec r{};
            r.L = La + Lb + Lc + Ld; r.nM = r.L / 2 + 1; r.tsize = (r.L + 1) * (r.L + 2) / 2;
            r.nT = (La + 1) * (Lb + 1) * (Lc + 1) * (Ld + 1); r.xz = r.nT * r.nM;
            const int Lab1 = La + Lb + 1;
            r.gsz = (Lc + 1) * (Ld + 1) * Lab1 * r.nM;
            r.lgG = 0; while ((1 << r.lgG) < r.gsz && (1 << r.lgG) < TF_ERI_THREADS) ++r.lgG;
            r.lgX = 0; while ((1 << r.lgX) < r.xz && (1 << r.lgX) < TF_ERI_THREADS) ++r.lgX;
            // batch capacity: the smallest over the launches (contracted bra and / or ket group) this tuple can occur in
            int nb = TF_ERI_THREADS / (r.L + 1);
            for (int fb = 0; fb < 2 && with_caps; ++fb)
                for (int fk = 0; fk < 2; ++fk) {
                    if (fb + fk == 0) continue;
                    const CFCaps &c = gcaps[2 * gb + fb][2 * gk + fk];
                    if (c.capR < 2 * r.tsize || c.capG < r.gsz || c.capXZ < r.xz) continue;   // (no such quartet in that launch)
                    nb = std::min(nb, c.capR / r.tsize - 1);
                    nb = std::min(nb, std::min(c.capG / r.gsz, c.capXZ / r.xz));
                }
            r.nb_cap = std::max(nb, 1);
            // entry e of the G table = ((cc (Ld + 1) + d) Lab1 + v) nM + n, of the X / Z tables = (((a2 (Lb + 1) + b2) (Lc + 1) + cc) (Ld + 1) + d) nM + m
            // (nested loops in that order: a cc-pVQZ basis has 625 tuples and 6e5 entries -- with a division chain per entry this was
            // 2 ms of every tensor build)
            r.tupG_off = (int)tup.size();
            tup.resize(tup.size() + (size_t)r.gsz + (size_t)r.xz);
            unsigned short *tp = tup.data() + r.tupG_off;
            for (int cc = 0; cc <= Lc; ++cc)
                for (int d = 0; d <= Ld; ++d)
                    for (int v = 0; v < Lab1; ++v)
                        for (int n = 0; n < r.nM; ++n) *tp++ = (unsigned short)(n | (v << 4) | (d << 8) | (cc << 11));
            r.tupXZ_off = r.tupG_off + r.gsz;
            for (int a2 = 0; a2 <= La; ++a2)
                for (int b2 = 0; b2 <= Lb; ++b2)
                    for (int cc = 0; cc <= Lc; ++cc)
                        for (int d = 0; d <= Ld; ++d)
                            for (int m = 0; m < r.nM; ++m) *tp++ = (unsigned short)(m | (a2 << 4) | (b2 << 7) | (cc << 10) | (d << 13));
            recs[ab * 36 + cd] = r;
        }
    if (ctx->d_lrec) { (void)tf_free(ctx->d_lrec); ctx->d_lrec = nullptr; }
    if (ctx->d_tup) { (void)tf_free(ctx->d_tup); ctx->d_tup = nullptr; }
    int rc2;
    if ((rc2 = upload(ctx, recs, &ctx->d_lrec, false)) || (rc2 = upload(ctx, tup, &ctx->d_tup, false))) return rc2;
    ctx->db.lrec = ctx->d_lrec; ctx->db.tup = ctx->d_tup;
    lrecs_host = recs;
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
        const auto key = std::make_pair(psid[pr.A], psid[pr.B]);
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
    static const bool old_generic = getenv("TF_ERI_GENERIC_OLD") != nullptr;
    struct Launch { size_t b0, b1; int gb, gk; double cost; };
    std::vector<Launch> launches;
    double ket_cost[NGRP];
    for (int g = 0; g < NGRP; ++g) {
        ket_cost[g] = 0.0;
        for (int k = kets_goff[g]; k < kets_goff[g + 1]; ++k) ket_cost[g] += (double)pair_cost(kets_all_host[k]);
    }
    for (size_t b0 = 0; b0 < bra_host.size();) {
        const int gb = pair_group(bra_host[b0]);
        size_t b1 = b0;
        double bc = 0.0;
        while (b1 < bra_host.size() && pair_group(bra_host[b1]) == gb) { bc += (double)pair_cost(bra_host[b1]); ++b1; }
        for (int gk = 0; gk < NGRP; ++gk)
            if (kets_goff[gk + 1] > kets_goff[gk]) launches.push_back(Launch{b0, b1, gb, gk, bc * ket_cost[gk]});
        b0 = b1;
    }
    std::stable_sort(launches.begin(), launches.end(), [](const Launch &x, const Launch &y) { return x.cost > y.cost; });
    // (as many streams as the process has hardware queues: 4 unless GPU_MAX_HW_QUEUES says otherwise -- tuna_amd sets 16)
    const int hwq = getenv("GPU_MAX_HW_QUEUES") ? std::max(1, atoi(getenv("GPU_MAX_HW_QUEUES"))) : 4;
    const int NQ = std::min(NSTREAM, getenv("TF_ERI_NQ") ? std::max(1, atoi(getenv("TF_ERI_NQ"))) : std::max(4, std::min(8, hwq)));
    std::vector<double> load(NQ, 0.0);
    BraFams bra_fams;
    for (const Launch &l : launches) {
        const int qi = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        load[qi] += l.cost;
        hipStream_t st = streams[qi];
        const int gb = l.gb, gk = l.gk, nk = kets_goff[gk + 1] - kets_goff[gk];
        const size_t b0 = l.b0, b1 = l.b1;
        const CFCaps &c = gcaps[gb][gk];
        const size_t bytes = (size_t)c.lds_doubles * sizeof(double);
        if (old_generic || !gcaps_fit[gb][gk]) {             // the component-per-lane kernel
            launch_generic_old((unsigned)(b1 - b0), d_bra + b0, d_braoff + b0, (unsigned)nk, d_kets_all + kets_goff[gk], st);
            continue;
        }
        if (bytes > 64 * 1024 && !ctx->cfact_lds_set) {
            HIPCHK(ctx, hipFuncSetAttribute((const void *)eri_cfact_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
            HIPCHK(ctx, hipFuncSetAttribute((const void *)eri_cfact_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
            HIPCHK(ctx, hipFuncSetAttribute((const void *)eri_cfact_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
            ctx->cfact_lds_set = 160 * 1024;
        }
        if (gcaps_gtab[gb][gk]) {
            const size_t need = (size_t)nk * (b1 - b0) * (size_t)c.gtab_doubles * sizeof(double);
            if (need > ctx->gtab_bytes) {
                HIPCHK(ctx, hipDeviceSynchronize());           // (earlier launches of this build may still use the old block)
                if (ctx->d_gtab) (void)tf_free(ctx->d_gtab);
                ctx->d_gtab = nullptr; ctx->gtab_bytes = 0;
                HIPCHK(ctx, tf_malloc((void **)&ctx->d_gtab, need));
                ctx->gtab_bytes = need;
            }
            // launches that share the block must not overlap: they all go to one stream
            count(TF_ERI_STAT_CFACT_GTAB);
            hipLaunchKernelGGL((eri_cfact_kernel<true, true>), dim3((unsigned)nk, (unsigned)(b1 - b0)), dim3(TF_ERI_THREADS), bytes, streams[0], ctx->db, c,
                               d_bra + b0, d_braoff + b0, d_kets_all + kets_goff[gk], Nc, d_C, ctx->d_gtab);
            load[qi] -= l.cost; load[0] += l.cost;
        } else if (((gb | gk) & 1) == 0) {                   // both groups uncontracted: one primitive quartet per shell quartet
            count(TF_ERI_STAT_CFACT_UNCONTRACTED);
            hipLaunchKernelGGL(eri_cfact_kernel<true>, dim3((unsigned)nk, (unsigned)(b1 - b0)), dim3(TF_ERI_THREADS), bytes, st, ctx->db, c,
                               d_bra + b0, d_braoff + b0, d_kets_all + kets_goff[gk], Nc, d_C);
        } else if ((gb & 1) && !(gk & 1) && bra_fam_on) {       // contracted bras against uncontracted kets: (family of bra pairs, ket pair).
            // Off by default (TF_ERI_BRA_FAMILIES=1): the packed layout evaluates the kets whose first shell does not exceed the bra's,
            // and the contracted shells come first on each atom -- the contracted pairs sit on the ket side; measured on Ar2/cc-pVQZ these
            // bra families cost 5 % (fewer, longer workgroups) where the ket families gain 24 %.
            const BraFam *bf = bra_families(bra_fams, bra_host, b0, b1, FAM_MM);
            if (!bf) return TF_ENOMEM;
            static bool bfam_attr_set = false;
            if (bytes > 64 * 1024 && !bfam_attr_set) {
                HIPCHK(ctx, hipFuncSetAttribute((const void *)eri_cfact_kernel<false, false, FAM_MM, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
                bfam_attr_set = true;
            }
            count(TF_ERI_STAT_CFACT_BRA_FAMILIES);
            hipLaunchKernelGGL((eri_cfact_kernel<false, false, FAM_MM, 1>), dim3((unsigned)nk, bf->n), dim3(TF_ERI_THREADS), bytes, st,
                               ctx->db, c, d_bra, d_braoff, d_kets_all + kets_goff[gk], Nc, d_C, (double *)nullptr, (const int *)nullptr,
                               (const int *)nullptr, bf->d_ptr, bf->d_mem);
        }
        else if ((gb & 1) && (gk & 1) && fam_any && !cc_fam_off) {
            // contracted against contracted: families on both sides -- up to 3 bra pairs x up to 9 ket pairs per workgroup (27 accumulators
            // per component: the deepest quartets, (s13 s13|s13 s13) and friends, spend their time in the tables of 28 561 primitive quartets)
            const BraFam *bf = bra_families(bra_fams, bra_host, b0, b1, FAM_MA_CC);
            if (!bf) return TF_ENOMEM;
            static bool ccfam_attr_set = false;
            if (bytes > 64 * 1024 && !ccfam_attr_set) {
                HIPCHK(ctx, hipFuncSetAttribute((const void *)eri_cfact_kernel<false, false, FAM_MA_CC, FAM_MM>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
                ccfam_attr_set = true;
            }
            count(TF_ERI_STAT_CFACT_BOTH_FAMILIES);
            hipLaunchKernelGGL((eri_cfact_kernel<false, false, FAM_MA_CC, FAM_MM>), dim3((unsigned)(fam_goff[gk + 1] - fam_goff[gk]), bf->n),
                               dim3(TF_ERI_THREADS), bytes, st, ctx->db, c, d_bra, d_braoff, d_fam_heads + fam_goff[gk], Nc, d_C, (double *)nullptr,
                               d_fam_ptr + fam_goff[gk], d_fam_mem, bf->d_ptr, bf->d_mem);
        }
        else if ((gk & 1) && fam_any) {                       // contracted kets: one workgroup per (bra pair, family of ket pairs)
            static bool fam_attr_set = false;                 // (per process and device: the attribute belongs to the function)
            if (bytes > 64 * 1024 && !fam_attr_set) {
                HIPCHK(ctx, hipFuncSetAttribute((const void *)eri_cfact_kernel<false, false, 1, FAM_MM>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
                fam_attr_set = true;
            }
            count(TF_ERI_STAT_CFACT_KET_FAMILIES);
            hipLaunchKernelGGL((eri_cfact_kernel<false, false, 1, FAM_MM>), dim3((unsigned)(fam_goff[gk + 1] - fam_goff[gk]), (unsigned)(b1 - b0)),
                               dim3(TF_ERI_THREADS), bytes, st, ctx->db, c, d_bra + b0, d_braoff + b0, d_fam_heads + fam_goff[gk], Nc, d_C,
                               (double *)nullptr, d_fam_ptr + fam_goff[gk], d_fam_mem);
        } else {
            count(TF_ERI_STAT_CFACT_CONTRACTED);
            hipLaunchKernelGGL(eri_cfact_kernel<false>, dim3((unsigned)nk, (unsigned)(b1 - b0)), dim3(TF_ERI_THREADS), bytes, st, ctx->db, c,
                               d_bra + b0, d_braoff + b0, d_kets_all + kets_goff[gk], Nc, d_C);
        }
        ++launch_count;
    }
    return TF_OK;
}

// ---- team kernels (tf_eri_team.hip.h): the uncontracted classes of the per-class mode, packed layout.  Per pair class the ket
// pair transform (Cartesian component pairs -> output pairs inside each x/y parity class, normalisation ratios folded in), per
// shell pair the slab offsets of its output pairs.
int EriBuild::plan_team_tables()
{
    int rc;
    if (!use_team) return TF_OK;
    std::vector<int> kt_ptr, kt_k, kq_ptr(npairs, 0), kq_off;
    std::vector<double> kt_c, blkC, blkD;
    std::vector<std::vector<int>> kap_list(ncls);               // output pairs (sc << 8 | sd) of a pair class, sorted by parity class
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
    for (int c = 0; c < ncls; ++c) {
        const DPair &pr = ctx->host_pairs[ctx->class_pairs[c][0]];
        const tf::Shell &sC = bs.shells[pr.A], &sD = bs.shells[pr.B];
        const int nsc = out_dim(sC), nsd = out_dim(sD), ncc = sC.ncomp, ncd = sD.ncomp;
        rows_of(sC, blkC); rows_of(sD, blkD);
        std::vector<int> loc((size_t)ncc * ncd, 0);              // position of a component pair inside its parity class (inverse of ct_ord)
        for (int cl = 0; cl < 4; ++cl)
            for (int s2 = pr.pcls[cl]; s2 < pr.pcls[cl + 1]; ++s2) loc[ctx->h_ct_ord[pr.tab_off + s2]] = s2 - pr.pcls[cl];
        KClassTab &kt = kct[c];
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
    for (int p = 0; p < npairs; ++p) {
        const DPair &pr = ctx->host_pairs[p];
        kq_ptr[p] = (int)kq_off.size();
        for (int word : kap_list[ctx->pair_class[p]]) {
            const int k = pr.outoff_a + (word >> 8), l = pr.outoff_b + (word & 255);
            if (l > k) { kq_off.push_back(-1); continue; }
            const int cb = H.cls[k] ^ H.cls[l];
            kq_off.push_back(H.fullsec[cb][H.cls[k]] + H.kinfo[(size_t)cb * N + H.sigma[k]].offA + H.loc[l]);
        }
    }
    if ((rc = mem.up(kq_ptr, &d_kq_ptr)) || (rc = mem.up(kq_off, &d_kq_off)) || (rc = mem.up(kt_ptr, &d_kt_ptr)) ||
        (rc = mem.up(kt_k, &d_kt_k)) || (rc = mem.up(kt_c, &d_kt_c)))
        return rc;
    ctx->db.kq_ptr = d_kq_ptr; ctx->db.kq_off = d_kq_off; ctx->db.kt_ptr = d_kt_ptr; ctx->db.kt_k = d_kt_k; ctx->db.kt_c = d_kt_c;
    // flat records of the class-sorted ket list (uncontracted pairs) and, per class and shell A, the kets with first shell <= A
    std::vector<KetRec> krec(ket_sorted.size());
    for (size_t k = 0; k < ket_sorted.size(); ++k) {
        const tf::Pair &pr = bs.pairs[ket_sorted[k]];
        const double qq = bs.pp_p[pr.pp_off];
        krec[k] = KetRec{qq, bs.pp_Pz[pr.pp_off], bs.pp_K[pr.pp_off] / qq, (unsigned)pr.e_off, kq_ptr[ket_sorted[k]]};
    }
    std::vector<int> kcnt((size_t)ncls * nsh, 0);
    for (int c = 0; c < ncls; ++c) {
        for (int p2 : ctx->class_pairs[c]) ++kcnt[(size_t)c * nsh + bs.pairs[p2].A];
        for (int a = 1; a < nsh; ++a) kcnt[(size_t)c * nsh + a] += kcnt[(size_t)c * nsh + a - 1];
    }
    if ((rc = mem.up(krec, &d_ketrec)) || (rc = mem.up(kcnt, &d_kcnt))) return rc;
    if (use_team_pc) {
        // flat lists of the parity-allowed components and of the outputs of every (bra class, ket class) of uncontracted pairs
        std::vector<int> tflat;
        flat_off.assign((size_t)ncls * ncls, -1);
        for (int bc = 0; bc < ncls; ++bc)
            for (int kc = 0; kc < ncls; ++kc) {
                const DPair &hb = ctx->host_pairs[ctx->class_pairs[bc][0]], &hk = ctx->host_pairs[ctx->class_pairs[kc][0]];
                if (hb.npp != 1 || hk.npp != 1 || hb.La + hb.Lb > TF_TEAM_LMAX || hk.La + hk.Lb > TF_TEAM_LMAX) continue;
                int mb, mk, nz;
                const TClass t = tclass_common(bc, kc, mb, mk, nz);
                if (nz > 2048) continue;                          // (chunked classes keep the loop per parity class)
                flat_off[(size_t)bc * ncls + kc] = (int)tflat.size();
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

// device index buffers sized for the largest possible slab, reused by every slab
int EriBuild::plan_index_buffers()
{
    int rc;
    size_t max_out = 0;
    for (int p : mine_sorted) max_out = std::max<size_t>(max_out, (size_t)pair_rows[p]);
    cap_bra = std::min<size_t>(mine_sorted.size(), 65535) + 1;
    cap_out = (size_t)std::min<long long>(ctx->n_rows, max_rows_c * 2 + (long long)max_out) + 1;
    // two sets of a slab's index lists: the lists of slab k + 1 are uploaded (on a stream of their own) while the kernels of slab k run;
    // the kernels themselves stay ordered by the streams (one half-transformed slab)
    out_bytes = cap_out * std::max(std::max(sizeof(OutRow), sizeof(OutRowP)), sizeof(OutRowT)); rowcls_bytes = (size_t)max_rows_c + 1;
    if ((rc = mem.alloc(&d_bra, 2 * cap_bra * sizeof(int)))) return rc;
    if ((rc = mem.alloc(&d_braoff, 2 * cap_bra * sizeof(long long)))) return rc;
    if (use_team_pc) if ((rc = mem.alloc(&d_brarec, 2 * cap_bra * sizeof(BraRec)))) return rc;
    if ((rc = mem.alloc(&d_out, 2 * out_bytes))) return rc;
    if (packed && !per_class) if ((rc = mem.alloc(&d_rowcls, 2 * rowcls_bytes))) return rc;
    d_bra_alloc = d_bra; d_braoff_alloc = d_braoff; d_out_alloc = d_out;
    d_brarec_alloc = d_brarec; d_rowcls_alloc = d_rowcls;
    d_bra_base = d_bra;
    return TF_OK;
}

// Generation: slab size, work counters, ket lists and families, streams, the launch tables of the mode, the slabs' index lists
int EriBuild::plan_generation()
{
    int rc;
    if ((rc = plan_slab_size())) return rc;
    plan_work_counters();
    DBG("slab buffers allocated");
    t_wall0 = std::chrono::steady_clock::now();
    if ((rc = plan_ket_lists()) || (rc = plan_ket_families())) return rc;
    // my bra pairs ordered by class: a slab is a run of that list, launches go per (bra class run, ket class)
    mine_sorted.clear();
    for (int c = 0; c < ncls; ++c)
        for (int p : ctx->class_pairs[c])
            if (owner[p] == ctx->rank) mine_sorted.push_back(p);
    if ((rc = setup_streams())) return rc;
    DBG("streams created");
    static const bool team_off = getenv("TF_ERI_TEAM") && getenv("TF_ERI_TEAM")[0] == '0';
    const bool team_ok = packed && !team_off && bs.epool.size() < 0xffffffffull;
    use_team_pc = team_ok && per_class;                                        // per-class mode: eri_team_kernel for the uncontracted classes
    // (off by default: on the BASELINE basis sets eri_cfact_kernel is faster -- N2/cc-pVTZ 1.2 ms against 3.3-4.2 ms, Ar2/cc-pVQZ 18 ms against
    // 22-25 ms of ERI kernels: a team walks the primitive quartets of its shell quartet one after the other, a chain of dependent phases
    // with nothing else on the chip to hide it; TF_ERI_TEAMC=1 switches it on for experiments and for the parity tests)
    static const bool teamc_off = !(getenv("TF_ERI_TEAMC") && getenv("TF_ERI_TEAMC")[0] == '1');
    use_teamc = team_ok && !per_class && !teamc_off;                          // small-problem mode: eri_teamc_kernel over task lists
    use_team = use_team_pc || use_teamc;                                       // the team kernels' tables are needed
    static const int teamc_pqmax_env = getenv("TF_TEAMC_PQMAX") ? atoi(getenv("TF_TEAMC_PQMAX")) : 700;
    teamc_pqmax = teamc_pqmax_env;
    kct.assign(ncls, KClassTab());
    DBG("stage: small-problem groups");
    DBG("stage: carve-outs");
    DBG("stage: launch lambda defined");
    if (!per_class) make_caps();
    DBG("stage: index-word tables");
    if ((rc = make_lrecs(!per_class))) return rc;
    DBG("stage: team tables");
    if ((rc = plan_team_tables())) return rc;
    if (!per_class)
        std::stable_sort(mine_sorted.begin(), mine_sorted.end(), [&](int x, int y) {
            const int gx = pair_group(x), gy = pair_group(y);
            return gx != gy ? gx < gy : pair_cost(x) > pair_cost(y);
        });
    if ((rc = plan_index_buffers())) return rc;
    DBG("stage: teamc tables");
    tc_of.assign((size_t)ncls * ncls, -2);
    for (int p2 = 0; p2 < npairs; ++p2) {
        any_wide_pair = any_wide_pair || bs.pairs[p2].La + bs.pairs[p2].Lb > TF_TEAM_LMAX;
        max_npp_all = std::max(max_npp_all, bs.pairs[p2].npp);
    }
    return TF_OK;
}

// ---- small-problem mode with team kernels (eri_teamc_kernel): class records per (bra class, ket class), created on demand; tasks
// per slab.  A quartet belongs to that kernel when both pair sums are <= TF_TEAM_LMAX and it has <= teamc_pqmax primitive quartets;
// eri_cfact_kernel skips exactly those (CFCaps::team_lmax / team_pqmax).
int EriBuild::teamc_class(int bcls, int kcls)
{
    int &slot = tc_of[(size_t)bcls * ncls + kcls];
    if (slot != -2) return slot;
    int maxblk, maxK, nnzc;
    TClass t = tclass_common(bcls, kcls, maxblk, maxK, nnzc);
    const int LAB = t.La + t.Lb, LCD = t.Lc + t.Ld, L = LAB + LCD, NM = L / 2 + 1, XS = NM | 1;
    if (LAB > TF_TEAM_LMAX || LCD > TF_TEAM_LMAX) return slot = -1;
    auto even = [](int x) { return (x + 1) & ~1; };
    int o = 0;
    t.oE12 = 0;
    t.oOffA = o; o += 2 * t.nab;
    t.oScA = o; o += even(t.nab);
    t.oOffK = o; o += 2 * t.ncd;
    t.oTp = o; o += even((t.nkap + 2) / 2);
    t.oTk = o; o += even((t.nnzT + 1) / 2);
    t.oTc = o; o += even(t.nnzT);
    t.shared_doubles = o;
    t.vcap = even(2 * t.nEab + 2 * t.nEcd + (L + 1) * (L + 2) + t.nTcd * (LAB + 1) * NM);      // E12, E34, R, G of one primitive quartet
    t.team_doubles = 2 * t.nT * XS + t.vcap + even(t.nacc) + even((t.nkap + 1) / 2);
    auto bytes_of = [&](int tm) { return ((size_t)t.shared_doubles + (size_t)(256 / tm) * t.team_doubles) * sizeof(double); };
    int team = 0;
    if (t.nT <= 16 && nnzc <= 96 && eri_team_available(LAB, LCD, 16)) team = 16;
    else if (eri_team_available(LAB, LCD, 64) && bytes_of(64) <= 52 * 1024) team = 64;
    else if (eri_team_available(LAB, LCD, 256) && bytes_of(256) <= 160 * 1024 - 256) team = 256;
    else if (eri_team_available(LAB, LCD, 64) && bytes_of(64) <= 160 * 1024 - 256) team = 64;
    if (!team) return slot = -1;
    tcs_host.push_back(t); tc_team.push_back(team); tc_lds.push_back(bytes_of(team));
    return slot = (int)tcs_host.size() - 1;
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
        for (int kc = 0; kc < ncls; ++kc) {
            const std::vector<int> &kl = ctx->class_pairs[kc];
            const int nk_all = (int)(std::upper_bound(kl.begin(), kl.end(), A, [&](int a, int p2) { return a < bs.pairs[p2].A; }) - kl.begin());
            if (nk_all == 0) continue;
            const int id = teamc_class(bcls, kc);
            if (id < 0) continue;
            const int team = tc_team[(size_t)id], NT = 256 / team;
            int lg = 10;
            while (((size_t)1 << lg) < tc_lds[(size_t)id]) ++lg;
            const std::array<int, 4> key{tcs_host[(size_t)id].La + tcs_host[(size_t)id].Lb, tcs_host[(size_t)id].Lc + tcs_host[(size_t)id].Ld, team, lg};
            auto it = lidx.find(key);
            if (it == lidx.end()) { it = lidx.emplace(key, (int)tcl.size()).first; tcl.push_back(TcLaunch{key[0], key[1], team, 0, {}, {}}); }
            TcLaunch &TL = tcl[(size_t)it->second];
            TL.lds = std::max(TL.lds, tc_lds[(size_t)id]);
            for (int g0 = 0; g0 < nk_all; g0 += NT) {
                const int nk = std::min(NT, nk_all - g0);
                int npq_max = 0, todo = 0;
                for (int u = 0; u < nk; ++u) {
                    const int npq = bs.pairs[pb].npp * bs.pairs[kl[(size_t)(g0 + u)]].npp;
                    if (npq <= teamc_pqmax) { ++todo; npq_max = std::max(npq_max, npq); }
                }
                if (!todo) continue;                       // (every quartet of the group goes to eri_cfact_kernel)
                TL.tasks.push_back(TeamTask{id, pb, ket_off[kc] + g0, nk, braoff[b]});
                TL.cost.push_back((double)npq_max * (tcs_host[(size_t)id].nT + tcs_host[(size_t)id].nacc));
            }
        }
    }
    old_needed = any_wide_pair || (long long)max_npp_bra * max_npp_all > teamc_pqmax;
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
    if (tcs_host.size() > d_tcs_cap) {
        mem.drop(d_tcs);
        d_tcs_cap = tcs_host.size() + 64;
        if ((rc = mem.alloc(&d_tcs, d_tcs_cap * sizeof(TClass)))) return rc;
    }
    if (all.size() > d_tasks_cap) {
        mem.drop(d_tasks);
        d_tasks_cap = all.size() + 1024;
        if ((rc = mem.alloc(&d_tasks, d_tasks_cap * sizeof(TeamTask)))) return rc;
    }
    if (!tcs_host.empty()) HIPCHK(ctx, hipMemcpy(d_tcs, tcs_host.data(), tcs_host.size() * sizeof(TClass), hipMemcpyHostToDevice));
    if (!all.empty()) HIPCHK(ctx, hipMemcpy(d_tasks, all.data(), all.size() * sizeof(TeamTask), hipMemcpyHostToDevice));
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
    for (auto &e : et) { if ((rc = mem.event(&e))) return rc; tev2.push_back(e); }
    HIPCHK(ctx, hipEventRecord(et[0], 0));
    HIPCHK(ctx, hipEventRecord(sev[0], 0));
    for (int k = 0; k < NSTREAM; ++k) HIPCHK(ctx, hipStreamWaitEvent(streams[k], sev[0], 0));
    int nl = 0;
    for (size_t k : order) {
        const TcLaunch &TL = tcl[k];
        if (TL.tasks.empty()) continue;
        TeamcLaunch a{TL.LAB, TL.LCD, TL.team, (unsigned)TL.tasks.size(), TL.lds, streams[nl++ % NSTREAM], &ctx->db, d_tcs, d_tasks + first[k], d_kets,
                      teamc_pqmax, d_T2};
        const hipError_t e = eri_teamc_launch(a);
        if (e != hipSuccess && team_error == hipSuccess) team_error = e;
        count(TF_ERI_STAT_TEAMC);
        ++launch_count;
    }
    for (int k = 0; k < NSTREAM; ++k) {
        HIPCHK(ctx, hipEventRecord(sev[k], streams[k]));
        HIPCHK(ctx, hipStreamWaitEvent(0, sev[k], 0));
    }
    HIPCHK(ctx, hipEventRecord(et[1], 0));
    return TF_OK;
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
    while (cursor < mine_sorted.size()) {
        const int p = mine_sorted[cursor];
        const tf::Shell &a = bs.shells[bs.pairs[p].A], &b = bs.shells[bs.pairs[p].B];
        const long long nr = (long long)a.ncomp * b.ncomp;
        if (!bra.empty() && (rows_c + nr > cut_rows || bra.size() >= 65535 || outs.size() + outsP.size() + outsT.size() + (size_t)pair_rows[p] >= cap_out)) break;
        bra.push_back(p); braoff.push_back(rows_c);
        long long r = rows.pair_first_row[p];
        for (int x = 0; x < out_dim(a); ++x)
            for (int y = 0; y < out_dim(b); ++y) {
                const int i = out_off(a) + x, j = out_off(b) + y;
                if (i < j) continue;
                if (!packed) { outs.push_back(OutRow{i, j, a.cart_off, b.cart_off, b.ncomp, 0, rows_c, r++}); continue; }
                if (tiles) { outsT.push_back(OutRowT{i, j, H.sigma[i], H.sigma[j], H.cls[i] ^ H.cls[j], b.ncomp, a.cart_off, b.cart_off, rows_c}); continue; }
                const int lr = rows.rowmap[tfp::ikey(H.sigma[i], H.sigma[j])];
                OutRowP o{};
                o.i = i; o.j = j; o.iI = H.sigma[i]; o.lamj = H.loc[j]; o.c = H.cls[i] ^ H.cls[j]; o.ncb = b.ncomp;
                o.cartA = a.cart_off; o.cartB = b.cart_off;
                for (int t = 0; t < 4; ++t) o.secoff[t] = rows.rowsec[6 * (size_t)lr + t];
                o.len = rows.rowlen[lr]; o.slab_off = rows_c; o.ubase = rows.rowoff[lr]; o.upos = rows.rowsec[6 * (size_t)lr + 4]; o.unr = rows.rowsec[6 * (size_t)lr + 5];
                outsP.push_back(o);
            }
        if (packed && !per_class)
            for (int ca = 0; ca < a.ncomp; ++ca)
                for (int cb = 0; cb < b.ncomp; ++cb) {
                    const int u = a.comp_off + ca, v = b.comp_off + cb;
                    rowcls.push_back((signed char)(((bs.c_lx[u] + bs.c_lx[v]) & 1) | (((bs.c_ly[u] + bs.c_ly[v]) & 1) << 1)));
                }
        rows_c += nr;
        const int Alim = packed ? bs.pairs[p].A + 1 : nsh;
        n_quart += cum_pairs[Alim];
        n_primq += (long long)bs.pairs[p].npp * cum_pp[Alim];
        n_compq += nr * cum_comp[Alim];
        {
            const double npp_ab = (double)bs.pairs[p].npp;
            const int lab = bs.pairs[p].La + bs.pairs[p].Lb;
            for (int c = 0; c < 4; ++c) {
                nominal_flops += 8.0 * npp_ab * pairW[p][c] * cumW[Alim][c];
                for (int lcd = 0; lcd <= 10; ++lcd) {
                    const double L1 = (double)(lab + lcd + 1);
                    nominal_flops += npp_ab * pairNc[p][c] * cumNL[Alim][4 * lcd + c] * (6.0 * L1 + 1.5 * L1 * L1 + 60.0);
                }
            }
        }
        ++cursor;
    }
    // this set of index lists was last read by the kernels of the slab before the previous one: wait for that slab only
    const int set = (int)(slab_no & 1);
    if (slab_no >= 2) HIPCHK(ctx, hipEventSynchronize(ctx->slab_done[set]));
    d_bra = d_bra_alloc + (size_t)set * cap_bra; d_braoff = d_braoff_alloc + (size_t)set * cap_bra;
    d_out = (char *)d_out_alloc + (size_t)set * out_bytes;
    if (d_brarec_alloc) d_brarec = d_brarec_alloc + (size_t)set * cap_bra;
    if (d_rowcls_alloc) d_rowcls = d_rowcls_alloc + (size_t)set * rowcls_bytes;
    d_bra_base = d_bra;
    ++slab_no;
    ++stats[TF_ERI_STAT_SLABS];
    const hipStream_t cst = ctx->cstream;
    HIPCHK(ctx, hipMemcpyAsync(d_bra, bra.data(), bra.size() * sizeof(int), hipMemcpyHostToDevice, cst));
    HIPCHK(ctx, hipMemcpyAsync(d_braoff, braoff.data(), braoff.size() * sizeof(long long), hipMemcpyHostToDevice, cst));
    std::vector<BraRec> brec;
    if (use_team_pc) {
        brec.resize(bra.size());
        for (size_t k = 0; k < bra.size(); ++k) {
            const tf::Pair &pr = bs.pairs[bra[k]];
            const double pp = bs.pp_p[pr.pp_off];
            brec[k] = BraRec{pp, bs.pp_Pz[pr.pp_off], bs.pp_K[pr.pp_off] / pp, (unsigned)pr.e_off, pr.A, braoff[k], 0};
        }
        HIPCHK(ctx, hipMemcpyAsync(d_brarec, brec.data(), brec.size() * sizeof(BraRec), hipMemcpyHostToDevice, cst));
    }
    if (!outs.empty()) HIPCHK(ctx, hipMemcpyAsync(d_out, outs.data(), outs.size() * sizeof(OutRow), hipMemcpyHostToDevice, cst));
    if (!outsP.empty()) HIPCHK(ctx, hipMemcpyAsync(d_out, outsP.data(), outsP.size() * sizeof(OutRowP), hipMemcpyHostToDevice, cst));
    if (!outsT.empty()) HIPCHK(ctx, hipMemcpyAsync(d_out, outsT.data(), outsT.size() * sizeof(OutRowT), hipMemcpyHostToDevice, cst));
    if (!rowcls.empty()) HIPCHK(ctx, hipMemcpyAsync(d_rowcls, rowcls.data(), rowcls.size(), hipMemcpyHostToDevice, cst));
    HIPCHK(ctx, hipStreamSynchronize(cst));                // (pageable sources: the copies are complete; the host vectors may go)
    DBG("slab: %zu bra pairs, %lld cart rows, %zu out rows", bra.size(), rows_c, outs.size() + outsP.size() + outsT.size());
    hipEvent_t e4[4];
    for (auto &e : e4) { if ((rc = mem.event(&e))) return rc; tev.push_back(e); }
    if (per_class && !packed && ld != N) HIPCHK(ctx, hipMemsetAsync(d_T2, 0, (size_t)rows_c * N * ld * sizeof(double), 0));   // pad columns
    std::vector<TcLaunch> tcl;
    bool old_needed = !use_teamc;
    if (use_teamc && (rc = teamc_tasks(bra, braoff, tcl, old_needed))) return rc;
    // generic mode: eri_cfact_kernel stores only the components that are not zero by x/y parity
    if (!per_class && old_needed) HIPCHK(ctx, hipMemsetAsync(d_C, 0, (size_t)rows_c * Nc * Nc * sizeof(double), 0));
    HIPCHK(ctx, hipEventRecord(e4[0], 0));
    for (int k = 0; k < NSTREAM; ++k) HIPCHK(ctx, hipStreamWaitEvent(streams[k], e4[0], 0));
    // runs of equal bra class inside the slab
    size_t r0 = 0;
    if (!per_class) { if (old_needed && (rc = launch_generic(bra, d_bra, d_braoff))) return rc; r0 = bra.size(); }
    while (r0 < bra.size()) {
        const int bcls = ctx->pair_class[bra[r0]];
        size_t r1 = r0;
        int max_npp = 1, Amax = 0;
        while (r1 < bra.size() && ctx->pair_class[bra[r1]] == bcls) {
            max_npp = std::max(max_npp, bs.pairs[bra[r1]].npp);
            Amax = std::max(Amax, bs.pairs[bra[r1]].A);
            ++r1;
        }
        for (int kcls = 0; kcls < ncls; ++kcls)
            launch_class(bcls, kcls, max_npp, (unsigned)(r1 - r0), d_bra + r0, d_braoff + r0, Amax);
        r0 = r1;
    }
    for (int k = 0; k < NSTREAM; ++k) {
        HIPCHK(ctx, hipEventRecord(sev[k], streams[k]));
        HIPCHK(ctx, hipStreamWaitEvent(0, sev[k], 0));
    }
    HIPCHK(ctx, hipEventRecord(e4[1], 0));
    if (!per_class && old_needed) {
        for (long long r0s = 0; r0s < rows_c; r0s += 65535) {      // both ket axes in one pass over the slab
            const unsigned ny = (unsigned)std::min<long long>(65535, rows_c - r0s);
            if (packed)
                hipLaunchKernelGGL(xform_ket_packed, dim3((unsigned)((N + 3) / 4), ny), dim3(256), 0, 0, d_C + (size_t)r0s * Nc * Nc,
                                   d_T2 + (size_t)r0s * H.RLS, Nc, ctx->bl, (long long)H.RLS, d_rowcls + r0s, ctx->d_csr_ptr, ctx->d_csr_idx,
                                   ctx->d_csr_val);
            else
                hipLaunchKernelGGL(xform_ket_both, dim3((unsigned)((N + 3) / 4), ny), dim3(256), 0, 0, d_C + (size_t)r0s * Nc * Nc,
                                   d_T2 + (size_t)r0s * N * ld, Nc, N, ld, ctx->d_csr_ptr, ctx->d_csr_idx, ctx->d_csr_val, 0);
        }
    }
    if (use_teamc && !tcl.empty() && (rc = launch_teamc(tcl))) return rc;
    HIPCHK(ctx, hipEventRecord(e4[2], 0));
    if (!outs.empty()) {
        const unsigned gx = (unsigned)std::min<long long>((row_len + 255) / 256, 4096);
        for (size_t o0 = 0; o0 < outs.size(); o0 += 65535) {
            const unsigned ny = (unsigned)std::min<size_t>(65535, outs.size() - o0);
            hipLaunchKernelGGL(xform_bra_store, dim3(gx, ny), dim3(256), 0, 0, d_T2, ctx->d_eri, reinterpret_cast<const OutRow *>(d_out) + o0,
                               row_len, ctx->d_csr_ptr, ctx->d_csr_idx, ctx->d_csr_val);
        }
    }
    if (!outsP.empty()) {
        int maxlen = 1;
        for (const OutRowP &o : outsP) maxlen = std::max(maxlen, o.len);
        for (size_t o0 = 0; o0 < outsP.size(); o0 += 65535) {
            const unsigned ny = (unsigned)std::min<size_t>(65535, outsP.size() - o0);
            hipLaunchKernelGGL(xform_bra_store_packed, dim3((unsigned)((maxlen + 255) / 256), ny), dim3(256), 0, 0, d_T2, ctx->d_eri,
                               reinterpret_cast<const OutRowP *>(d_out) + o0, (long long)H.RLS, ctx->bl, ctx->d_csr_ptr, ctx->d_csr_idx,
                               ctx->d_csr_val);
        }
    }
    if (!outsT.empty()) {
        for (size_t o0 = 0; o0 < outsT.size(); o0 += 65535) {
            const unsigned ny = (unsigned)std::min<size_t>(65535, outsT.size() - o0);
            hipLaunchKernelGGL(xform_bra_store_tiles, dim3((unsigned)((H.RLS + 255) / 256), ny), dim3(256), 0, 0, d_T2, ctx->d_eri,
                               reinterpret_cast<const OutRowT *>(d_out) + o0, (long long)H.RLS, ctx->bl, ctx->tv, ctx->d_csr_ptr, ctx->d_csr_idx,
                               ctx->d_csr_val);
        }
    }
    HIPCHK(ctx, hipEventRecord(e4[3], 0));
    HIPCHK(ctx, hipEventRecord(ctx->slab_done[set], 0));
    return TF_OK;
}

// Behind the last launch: drain the device, read the timing events, release the lists of the build, publish timings and counters
int EriBuild::finish()
{
    HIPCHK(ctx, hipDeviceSynchronize());
    DBG("device drained");
    HIPCHK(ctx, hipGetLastError());
    for (size_t k = 0; k + 3 < tev.size(); k += 4) {
        t_stage[1] += seconds_between(tev[k], tev[k + 1]);
        t_stage[2] += seconds_between(tev[k + 1], tev[k + 2]);
        t_stage[3] += seconds_between(tev[k + 2], tev[k + 3]);
    }
    for (size_t k = 0; k + 1 < tev2.size(); k += 2) {
        const double dt = seconds_between(tev2[k], tev2[k + 1]);
        t_stage[1] += dt; t_stage[2] -= dt;
    }
    mem.release();
    if (team_error != hipSuccess) TF_FAIL(ctx, TF_ENODEVICE, "launch of a team ERI kernel failed: %s", hipGetErrorString(team_error));
    t_stage[0] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_wall0).count();
    std::copy(t_stage, t_stage + 4, ctx->eri_seconds);
    ctx->eri_counts[0] = n_quart; ctx->eri_counts[1] = n_primq; ctx->eri_counts[2] = n_compq;
    ctx->eri_nominal_flops = nominal_flops;
    std::copy(stats, stats + TF_ERI_STAT_COUNT, ctx->eri_stats);
    return TF_OK;
}

}  // extern "C++"

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
    if ((rc = B.plan_storage())) return rc;
    DBG("rows=%lld N=%d ld=%d (tensor + row tables allocated)", ctx->n_rows, B.N, B.ld);
    if ((rc = B.plan_generation())) return rc;
    DBG("stage: slab loop");
    while (B.cursor < B.mine_sorted.size())
        if ((rc = B.run_slab())) return rc;
    DBG("all slabs launched (%d class launches)", B.launch_count);
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
        hipLaunchKernelGGL(expand_dense_tiles_kernel, dim3(g), dim3(256), 0, 0, ctx->d_eri, ctx->tv, ctx->bl, d_dense);
    else if (ctx->layout == 1)
        hipLaunchKernelGGL(expand_dense_packed_kernel, dim3(g), dim3(256), 0, 0, ctx->d_eri, ctx->d_rowmap, ctx->d_rowoff, ctx->d_rowsec, ctx->bl, d_dense);
    else
        hipLaunchKernelGGL(expand_dense_kernel, dim3(g), dim3(256), 0, 0, ctx->d_eri, ctx->d_rowmap, ctx->N, ctx->ld, d_dense);
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
        hipLaunchKernelGGL(sample_tiles_kernel, dim3((unsigned)((n_idx + 255) / 256)), dim3(256), 0, 0, ctx->d_eri, ctx->tv, ctx->bl, (long long)n_idx, d_idx, d_val);
    else if (ctx->layout == 1)
        hipLaunchKernelGGL(sample_packed_kernel, dim3((unsigned)((n_idx + 255) / 256)), dim3(256), 0, 0, ctx->d_eri, ctx->d_rowmap,
                           ctx->d_rowoff, ctx->d_rowsec, ctx->bl, (long long)n_idx, d_idx, d_val);
    else
        hipLaunchKernelGGL(sample_kernel, dim3((unsigned)((n_idx + 255) / 256)), dim3(256), 0, 0, ctx->d_eri, ctx->d_rowmap, ctx->N,
                           ctx->ld, (long long)n_idx, d_idx, d_val);
    hipError_t e = hipMemcpy(values, d_val, (size_t)n_idx * sizeof(double), hipMemcpyDeviceToHost);
    (void)tf_free(d_idx); (void)tf_free(d_val);
    HIPCHK(ctx, e);
    return TF_OK;
}

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

int tf_dft_clear(tf_ctx *ctx)
{
    if (!ctx) return TF_EINVAL;
    (void)hipSetDevice(ctx->device);
    tfdft::release(ctx->grid);
    return TF_OK;
}

int tf_dft_setup(tf_ctx *ctx, int64_t n_points, const double *xyz, const double *weights, int x_functional, int c_functional, double dfx,
                 double dfc, double x_alpha)
{
    if (!ctx) return TF_EINVAL;
    if (!ctx->have_eri) TF_FAIL(ctx, TF_EINVAL, "tf_dft_setup: call tf_build_eri first (it fixes the AO representation)");
    if (n_points < 1 || !xyz || !weights || x_functional < 0 || x_functional > 3 || c_functional < 0 || c_functional > 5)
        TF_FAIL(ctx, TF_EINVAL, "tf_dft_setup: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    tfdft::release(ctx->grid);
    tfdft::Grid &g = ctx->grid;
    const tf::Basis &bs = ctx->bs;
    const int N = ctx->N;
    const long long G = n_points;
    g.G = G; g.N = N; g.xid = x_functional; g.cid = c_functional; g.dfx = dfx; g.dfc = dfc; g.x_alpha = x_alpha;
    g.gga = (x_functional >= tfdft::X_B88) || (c_functional >= tfdft::C_LYP);
    std::string err;
    tfone::DevBuf buf;
    tfone::DAO A = tfone::upload_aos(bs, buf, err);
    if (!err.empty()) TF_FAIL(ctx, TF_ENODEVICE, "%s", err.c_str());
    double *d_xyz = buf.alloc<double>((size_t)3 * G, err);
    if (!err.empty()) TF_FAIL(ctx, TF_ENOMEM, "%s", err.c_str());
    HIPCHK(ctx, hipMemcpy(d_xyz, xyz, (size_t)3 * G * sizeof(double), hipMemcpyHostToDevice));
    const size_t GN = (size_t)G * N;
    // (the grid's buffers are released by tfdft::release in tf_dft.hip.h with the runtime's own hipFree: they bypass this file's block cache)
    HIPCHK(ctx, ::hipMalloc((void **)&g.w, (size_t)G * sizeof(double)));
    HIPCHK(ctx, hipMemcpy(g.w, weights, (size_t)G * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(ctx, ::hipMalloc((void **)&g.phi, GN * sizeof(double)));
    HIPCHK(ctx, ::hipMalloc((void **)&g.dphi, (g.gga ? 3 : 1) * GN * sizeof(double)));
    HIPCHK(ctx, ::hipMalloc((void **)&g.B, GN * sizeof(double)));
    HIPCHK(ctx, ::hipMalloc((void **)&g.D, GN * sizeof(double)));
    for (double **p : {&g.rho, &g.vrho, &g.vsig, &g.ex, &g.ec}) HIPCHK(ctx, ::hipMalloc((void **)p, (size_t)G * sizeof(double)));
    HIPCHK(ctx, ::hipMalloc((void **)&g.grad, (size_t)3 * G * sizeof(double)));
    HIPCHK(ctx, ::hipMalloc((void **)&g.V, (size_t)(tfdft::VSPLIT + 2) * N * N * sizeof(double)));
    HIPCHK(ctx, ::hipMalloc((void **)&g.part, (size_t)3 * tfdft::NPART * sizeof(double)));
    tfdft::DAOs D{A.z, A.lmn, A.prim_off, A.exps, A.w};
    hipLaunchKernelGGL(tfdft::ao_on_grid_kernel, dim3((unsigned)((GN + 127) / 128)), dim3(128), 0, 0, D, d_xyz, G, N, ctx->d_csr_ptr,
                       ctx->d_csr_idx, ctx->d_csr_val, g.phi, g.dphi, g.gga ? 1 : 0);
    HIPCHK(ctx, hipDeviceSynchronize());
    HIPCHK(ctx, hipGetLastError());
    std::string msg;
    int rc = tfscf::ensure(ctx->scf, N, 6, msg);           // makes sure the rocBLAS handle exists
    if (rc) { ctx->err = msg; return rc; }
    return TF_OK;
}

int tf_dft_vxc(tf_ctx *ctx, const double *P, double *Vxc, double *n_elec, double *e_x, double *e_c)
{
    if (!ctx) return TF_EINVAL;
    if (ctx->grid.G <= 0) TF_FAIL(ctx, TF_EINVAL, "tf_dft_vxc: call tf_dft_setup first");
    if (!ctx->have_eri || ctx->grid.N != ctx->N)
        TF_FAIL(ctx, TF_EINVAL, "tf_dft_vxc: the grid was set up for a different tensor (call tf_build_eri, then tf_dft_setup again)");
    if (!P || !Vxc) TF_FAIL(ctx, TF_EINVAL, "tf_dft_vxc: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)ctx->N * ctx->N;
    HIPCHK(ctx, hipMemcpy(ctx->jk.all.P, P, nn * sizeof(double), hipMemcpyHostToDevice));
    std::string msg;
    double o3[3];
    int rc = tfdft::vxc(ctx->scf.blas, ctx->grid, ctx->jk.all.P, ctx->jk.all.J, o3, msg);
    if (rc) { ctx->err = msg; return rc; }
    HIPCHK(ctx, hipMemcpy(Vxc, ctx->jk.all.J, nn * sizeof(double), hipMemcpyDeviceToHost));
    if (n_elec) *n_elec = o3[0];
    if (e_x) *e_x = o3[1];
    if (e_c) *e_c = o3[2];
    return TF_OK;
}

int tf_dft_vxc_unrestricted(tf_ctx *ctx, const double *P_alpha, const double *P_beta, double *Vxc_alpha, double *Vxc_beta, double n_elec[2],
                            double e_x[2], double *e_c)
{
    if (!ctx) return TF_EINVAL;
    if (ctx->grid.G <= 0) TF_FAIL(ctx, TF_EINVAL, "tf_dft_vxc_unrestricted: call tf_dft_setup first");
    if (!ctx->have_eri || ctx->grid.N != ctx->N)
        TF_FAIL(ctx, TF_EINVAL, "tf_dft_vxc_unrestricted: the grid was set up for a different tensor (call tf_build_eri, then tf_dft_setup again)");
    if (!P_alpha || !P_beta || !Vxc_alpha || !Vxc_beta) TF_FAIL(ctx, TF_EINVAL, "tf_dft_vxc_unrestricted: bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::string msg;
    int rc = tfdft::ensure_spin(ctx->grid, msg);
    if (rc) { ctx->err = msg; return rc; }
    const size_t nn = (size_t)ctx->N * ctx->N;
    double *io = ctx->grid.sio;                                  // P_alpha, P_beta, V_alpha, V_beta
    HIPCHK(ctx, hipMemcpy(io, P_alpha, nn * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(io + nn, P_beta, nn * sizeof(double), hipMemcpyHostToDevice));
    double o5[5];
    rc = tfdft::vxc_unrestricted(ctx->scf.blas, ctx->grid, io, io + nn, io + 2 * nn, io + 3 * nn, o5, msg);
    if (rc) { ctx->err = msg; return rc; }
    HIPCHK(ctx, hipMemcpy(Vxc_alpha, io + 2 * nn, nn * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(Vxc_beta, io + 3 * nn, nn * sizeof(double), hipMemcpyDeviceToHost));
    if (n_elec) { n_elec[0] = o5[0]; n_elec[1] = o5[1]; }
    if (e_x) { e_x[0] = o5[2]; e_x[1] = o5[3]; }
    if (e_c) *e_c = o5[4];
    return TF_OK;
}

// ---- AO->MO transformation, MP2 ... CCSD(T), CIS / TDHF: the drivers of the correlated methods (consumers of the resident tensor) ----
#include "tf_corr_host.hip.h"

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
    const tfscf::Workspace &w = ctx->scf;
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
        if (ctx->grid.N != ctx->N) TF_FAIL(ctx, TF_EINVAL, "tf_scf_rhf: the DFT grid was set up for a different AO dimension");
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
    if (ctx->grid.G <= 0) TF_FAIL(ctx, TF_EINVAL, "tf_scf_uks: call tf_dft_setup first (unrestricted Hartree-Fock is tf_scf_uhf)");
    if (ctx->grid.N != ctx->N) TF_FAIL(ctx, TF_EINVAL, "tf_scf_uks: the DFT grid was set up for a different AO dimension");
    if (ctx->world > 1) TF_FAIL(ctx, TF_EINVAL, "tf_scf_uks: unrestricted Kohn-Sham runs on an unsharded tensor (world = 1) in this build");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::string msg;
    tfscf::XC2Fn xc = [&](const double *dPa, const double *dPb, double *dVa, double *dVb, double *o5) {
        return tfdft::vxc_unrestricted(ctx->scf.blas, ctx->grid, dPa, dPb, dVa, dVb, o5, msg);
    };
    return scf_unrestricted(ctx, opts, S, T, V, Fext, X, P0_alpha, P0_beta, E0, n_alpha, n_beta, V_NN, out, msg, xc);
}

}  // extern "C"
