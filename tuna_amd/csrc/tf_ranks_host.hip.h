// tf_ranks_host.hip.h -- the ranks of a sharded tensor: RCCL loaded on demand, the communicator of a context and
// its one way out (comm_release), the sums over the ranks, the agreement on control decisions, and the entry points tf_set_allreduce,
// tf_comm_* and tf_shard_plan* (the plans themselves: tf_shard_plan.h).  Included by tf_device.hip below tf_ctx.hip.h; one translation unit.

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

// The one way a context lets go of its communicator: nothing queued on the device may still use it when it is destroyed.
static void comm_release(tf_ctx *ctx)
{
    if (!ctx->comm) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    (void)tfrccl::CommDestroy(ctx->comm);
    ctx->comm = nullptr;
}

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
    if (ctx->blk.ensure(CB_AGREE, 16 * sizeof(double)) != 0) { msg = "hipMalloc failed (agree buffer)"; return TF_ENOMEM; }
    if (hipMemcpy(ctx->d_agree(), h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess) { msg = "hipMemcpy failed (agree buffer)"; return TF_ENODEVICE; }
    int rc;
    if (ctx->comm) { rc = comm_allreduce(ctx, ctx->d_agree(), 16, nullptr); if (rc) { msg = ctx->err; return rc; } }
    else rc = ctx->allreduce(ctx->allreduce_user, ctx->d_agree(), 16, nullptr);
    if (rc) { msg = "the registered all-reduce failed (code " + std::to_string(rc) + ")"; return TF_ENODEVICE; }
    double s[16];
    if (hipMemcpy(s, ctx->d_agree(), sizeof(s), hipMemcpyDeviceToHost) != hipSuccess) { msg = "hipMemcpy failed (agree buffer)"; return TF_ENODEVICE; }
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

extern "C" {

int tf_shard_plan_pairs(int n_shells, const int32_t *dim, int layout, int world, int32_t *owner)
{
    if (n_shells < 0 || world < 1 || !dim || !owner || layout < 0 || layout > 1) return TF_EINVAL;
    std::vector<int> d(dim, dim + n_shells), o;
    shard_plan_pairs(d, layout >= 1, world, getenv("TF_SHARD_PLAN"), o);
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
    comm_release(ctx);
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
    comm_release(ctx);
    return TF_OK;
}

int tf_comm_attached(const tf_ctx *ctx) { return (ctx && ctx->comm) ? 1 : 0; }

}  // extern "C"
