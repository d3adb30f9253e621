// The context, its error strings, device memory, the layout transposes and RCCL (include/allocnet_amd.h).
#include <dlfcn.h>
#include <stdlib.h>
#include <new>

#include "api_internal.h"
#include "layout_kernels.h"

thread_local std::string g_err;

int ensure_counter(anet_ctx *ctx) {
  if (!ctx->d_counter) ANET_HIP(ctx, hipMalloc((void **)&ctx->d_counter, sizeof(int)));
  if (!ctx->h_counter) ANET_HIP(ctx, hipHostMalloc((void **)&ctx->h_counter, 2 * sizeof(int), hipHostMallocDefault));
  for (int i = 0; i < 2; ++i)
    if (!ctx->poll_ev[i]) ANET_HIP(ctx, hipEventCreateWithFlags(&ctx->poll_ev[i], hipEventDisableTiming));
  return ANET_OK;
}

extern "C" {

int anet_abi_version(void) { return ANET_ABI_VERSION; }

int anet_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int anet_compute_units(const anet_ctx *ctx) { return ctx ? ctx->cus : 0; }

int anet_create(int device, anet_ctx **out) {
  if (!out) return fail(nullptr, ANET_ERR_INVALID, "anet_create: out is NULL");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(nullptr, ANET_ERR_NODEVICE,
                "anet_create: no HIP device visible (this library has no CPU fallback)");
  if (device < 0 || device >= n) return fail(nullptr, ANET_ERR_INVALID, "anet_create: bad device index");
  anet_ctx *ctx = new (std::nothrow) anet_ctx();
  if (!ctx) return fail(nullptr, ANET_ERR_NOMEM, "anet_create: out of host memory");
  ctx->device = device;
  e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
  if (e == hipSuccess) {
    int cus = 0;
    e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e == hipSuccess && cus > 0) ctx->cus = cus;
  }
  if (e != hipSuccess) {
    int rc = hip_fail(nullptr, e, "anet_create");
    delete ctx;
    return rc;
  }
  *out = ctx;
  return ANET_OK;
}

void anet_destroy(anet_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->scratch) (void)hipFree(ctx->scratch);
  if (ctx->comm) (void)anet_comm_destroy(ctx);
  if (ctx->d_counter) (void)hipFree(ctx->d_counter);
  for (auto &t : ctx->tabs) {
    if (t.d) (void)hipFree(t.d);
    if (t.ready) (void)hipEventDestroy(t.ready);
  }
  for (auto &t : ctx->ipm_tabs) {
    if (t.d) (void)hipFree(t.d);
    if (t.ready) (void)hipEventDestroy(t.ready);
  }
  if (ctx->h_counter) (void)hipHostFree(ctx->h_counter);
  for (int i = 0; i < 2; ++i)
    if (ctx->poll_ev[i]) (void)hipEventDestroy(ctx->poll_ev[i]);
  if (ctx->h_pack) (void)hipHostFree(ctx->h_pack);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

const char *anet_last_error(const anet_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

void *anet_stream(anet_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int anet_synchronize(anet_ctx *ctx) {
  if (!ctx) return fail(nullptr, ANET_ERR_INVALID, "anet_synchronize: ctx is NULL");
  ANET_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ANET_OK;
}

int64_t anet_recommended_ld(int64_t batch) {
  int64_t ld = round_up(batch < 1 ? 1 : batch, 64);
  if (ld % 512 == 0) ld += 576;  // 512 doubles = 4 KiB: break (near-)power-of-two row strides
  return ld;
}

int anet_dev_alloc(anet_ctx *ctx, size_t n_doubles, double **out) {
  if (!ctx || !out) return fail(ctx, ANET_ERR_INVALID, "anet_dev_alloc: NULL argument");
  *out = nullptr;
  ANET_ON_DEVICE(ctx);
  hipError_t e = hipMalloc((void **)out, sizeof(double) * (n_doubles ? n_doubles : 1));
  if (e != hipSuccess) return fail(ctx, ANET_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
  return ANET_OK;
}
void anet_dev_free(double *p) {
  if (p) (void)hipFree(p);
}
int anet_dev_upload(anet_ctx *ctx, double *dst_dev, const double *src_host, size_t n_doubles) {
  if (!ctx || !dst_dev || !src_host) return fail(ctx, ANET_ERR_INVALID, "anet_dev_upload: NULL argument");
  ANET_ON_DEVICE(ctx);
  ANET_HIP(ctx, hipMemcpyAsync(dst_dev, src_host, sizeof(double) * n_doubles, hipMemcpyHostToDevice, ctx->stream));
  ANET_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ANET_OK;
}
int anet_dev_download(anet_ctx *ctx, double *dst_host, const double *src_dev, size_t n_doubles) {
  if (!ctx || !dst_host || !src_dev) return fail(ctx, ANET_ERR_INVALID, "anet_dev_download: NULL argument");
  ANET_ON_DEVICE(ctx);
  ANET_HIP(ctx, hipMemcpyAsync(dst_host, src_dev, sizeof(double) * n_doubles, hipMemcpyDeviceToHost, ctx->stream));
  ANET_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ANET_OK;
}

int anet_to_batch_minor_dev(anet_ctx *ctx, int64_t batch, int64_t nfield, int64_t ld,
                            const double *src, double *dst, void *stream) {
  ANET_ON_DEVICE(ctx);
  if (!ctx || !src || !dst || batch < 0 || nfield < 0 || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_to_batch_minor_dev: bad argument");
  if (batch == 0 || nfield == 0) return ANET_OK;
  dim3 grid((unsigned)((batch + anet::kTile - 1) / anet::kTile),
            (unsigned)((nfield + anet::kTile - 1) / anet::kTile));
  hipLaunchKernelGGL(anet::k_to_batch_minor, grid, dim3(anet::kTile, 8), 0, (hipStream_t)stream, src,
                     dst, batch, nfield, ld);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

int anet_to_traj_major_dev(anet_ctx *ctx, int64_t batch, int64_t nfield, int64_t ld,
                           const double *src, double *dst, void *stream) {
  ANET_ON_DEVICE(ctx);
  if (!ctx || !src || !dst || batch < 0 || nfield < 0 || ld < batch)
    return fail(ctx, ANET_ERR_INVALID, "anet_to_traj_major_dev: bad argument");
  if (batch == 0 || nfield == 0) return ANET_OK;
  dim3 grid((unsigned)((batch + anet::kTile - 1) / anet::kTile),
            (unsigned)((nfield + anet::kTile - 1) / anet::kTile));
  hipLaunchKernelGGL(anet::k_to_traj_major, grid, dim3(anet::kTile, 8), 0, (hipStream_t)stream, src,
                     dst, batch, nfield, ld);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

// ---- RCCL (loaded at run time) -------------------------------------------------------------------
namespace {
struct RcclApi {
  void *handle = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
RcclApi g_rccl;
int load_rccl(anet_ctx *ctx) {
  if (g_rccl.handle) return ANET_OK;
  const char *env = getenv("ANET_RCCL_PATH");
  const char *cands[] = {env, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so"};
  void *h = nullptr;
  for (const char *c : cands) {
    if (!c || !*c) continue;
    h = dlopen(c, RTLD_NOW | RTLD_GLOBAL);
    if (h) break;
  }
  if (!h) return fail(ctx, ANET_ERR_UNSUPPORTED, std::string("cannot load librccl.so: ") + dlerror());
  RcclApi a;
  a.handle = h;
  a.GetUniqueId = (decltype(a.GetUniqueId))dlsym(h, "ncclGetUniqueId");
  a.CommInitRank = (decltype(a.CommInitRank))dlsym(h, "ncclCommInitRank");
  a.AllGather = (decltype(a.AllGather))dlsym(h, "ncclAllGather");
  a.CommDestroy = (decltype(a.CommDestroy))dlsym(h, "ncclCommDestroy");
  a.GetErrorString = (decltype(a.GetErrorString))dlsym(h, "ncclGetErrorString");
  if (!a.GetUniqueId || !a.CommInitRank || !a.AllGather || !a.CommDestroy)
    return fail(ctx, ANET_ERR_UNSUPPORTED, "librccl.so lacks the expected nccl* symbols");
  g_rccl = a;
  return ANET_OK;
}
int rccl_fail(anet_ctx *ctx, ncclResult_t r, const char *what) {
  return fail(ctx, ANET_ERR_HIP, std::string(what) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "rccl error"));
}
}  // namespace

int anet_comm_unique_id(anet_ctx *ctx, unsigned char id[ANET_COMM_ID_BYTES]) {
  if (!ctx || !id) return fail(ctx, ANET_ERR_INVALID, "anet_comm_unique_id: NULL argument");
  int rc = load_rccl(ctx);
  if (rc) return rc;
  static_assert(sizeof(ncclUniqueId) == ANET_COMM_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId u;
  ncclResult_t r = g_rccl.GetUniqueId(&u);
  if (r != ncclSuccess) return rccl_fail(ctx, r, "ncclGetUniqueId");
  memcpy(id, &u, ANET_COMM_ID_BYTES);
  return ANET_OK;
}

int anet_comm_init(anet_ctx *ctx, int nranks, int rank, const unsigned char id[ANET_COMM_ID_BYTES]) {
  if (!ctx || !id || nranks < 1 || rank < 0 || rank >= nranks) return fail(ctx, ANET_ERR_INVALID, "anet_comm_init: bad argument");
  if (ctx->comm) return fail(ctx, ANET_ERR_INVALID, "anet_comm_init: communicator already initialised");
  int rc = load_rccl(ctx);
  if (rc) return rc;
  ANET_ON_DEVICE(ctx);
  ncclUniqueId u;
  memcpy(&u, id, ANET_COMM_ID_BYTES);
  ncclResult_t r = g_rccl.CommInitRank(&ctx->comm, nranks, u, rank);
  if (r != ncclSuccess) {
    ctx->comm = nullptr;
    return rccl_fail(ctx, r, "ncclCommInitRank");
  }
  ctx->comm_ranks = nranks;
  return ANET_OK;
}

int anet_comm_allgather_costs_dev(anet_ctx *ctx, const double *send, double *recv, int64_t count, void *stream) {
  ANET_ON_DEVICE(ctx);
  if (!ctx || !ctx->comm) return fail(ctx, ANET_ERR_INVALID, "anet_comm_allgather_costs_dev: call anet_comm_init first");
  if (!send || !recv || count < 0) return fail(ctx, ANET_ERR_INVALID, "anet_comm_allgather_costs_dev: bad argument");
  if (count == 0) return ANET_OK;
  ncclResult_t r = g_rccl.AllGather(send, recv, (size_t)count, ncclFloat64, ctx->comm, (hipStream_t)stream);
  if (r != ncclSuccess) return rccl_fail(ctx, r, "ncclAllGather");
  return ANET_OK;
}

int anet_comm_destroy(anet_ctx *ctx) {
  if (!ctx) return ANET_ERR_INVALID;
  if (ctx->comm && g_rccl.CommDestroy) {
    (void)g_rccl.CommDestroy(ctx->comm);
    ctx->comm = nullptr;
    ctx->comm_ranks = 0;
  }
  return ANET_OK;
}

}  // extern "C"
