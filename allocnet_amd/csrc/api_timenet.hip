// The time-allocation network: weights handle, batched inference (include/allocnet_amd.h, csrc/timenet_kernels.h).
#include "api_internal.h"
#include "timenet_kernels.h"

struct anet_timenet {
  anet_ctx *ctx = nullptr;  // compared only, never dereferenced: the handle may outlive it
  int device = -1;
  int seq_len = 0;
  float *d_weights = nullptr;  // the small tensors, then the packed recurrent operand: one allocation
  size_t weight_bytes = 0;
  anet::TimeNetWeights w{};
  float *xw = nullptr;  // [cap][40]: the encoders' output of the tile form, grow-only
  int64_t xw_cap = 0;
  void *stage = nullptr;  // device staging of the host entry point, grow-only
  size_t stage_bytes = 0;
};

namespace {

// tensor order of anet_timenet_create and element counts (flat = 16 (L / 4))
enum { SC_W, SC_B, SF_W, SF_B, HC_W, HC_B, HF_W, HF_B, W_IH, W_HH, B_IH, B_HH, T_W, T_B, S_W, S_B, N_TENSORS };

int check_forward(anet_ctx *ctx, const anet_timenet *net, int seq_len, int64_t batch, int flags) {
  if (!net) return fail(ctx, ANET_ERR_INVALID, "anet_timenet handle is NULL");
  if (net->ctx != ctx) return fail(ctx, ANET_ERR_INVALID, "anet_timenet: the handle belongs to another context");
  if (seq_len != net->seq_len) return fail(ctx, ANET_ERR_INVALID, "anet_timenet: seq_len differs from the handle's");
  if (batch < 0) return fail(ctx, ANET_ERR_INVALID, "negative batch");
  if (batch > (int64_t)INT32_MAX / 4) return fail(ctx, ANET_ERR_INVALID, "anet_timenet: batch too large for one launch");
  if ((flags & ANET_TIMENET_FORM_SINGLE) && (flags & ANET_TIMENET_FORM_TILE))
    return fail(ctx, ANET_ERR_INVALID, "anet_timenet: both kernel forms requested");
  return ANET_OK;
}

template <int L>
int launch(anet_ctx *ctx, anet_timenet *net, int64_t batch, const float *state, const float *hpolys, int flags,
           const anet::TimeNetOut &out, hipStream_t st) {
  const int skip = (flags & ANET_TIMENET_KEEP_PADDING) ? 0 : 1;
  const bool single = (flags & ANET_TIMENET_FORM_SINGLE) || (!(flags & ANET_TIMENET_FORM_TILE) && batch <= ANET_TIMENET_SINGLE_MAX);
  if (single) {
    hipLaunchKernelGGL(anet::k_timenet_single<L>, dim3((unsigned)batch), dim3(256), 0, st, net->w, state, hpolys, batch, skip, out);
    ANET_HIP(ctx, hipGetLastError());
    return ANET_OK;
  }
  if (batch > net->xw_cap) {  // only the first call at a larger batch allocates
    if (net->xw) ANET_HIP(ctx, hipFree(net->xw));
    net->xw = nullptr;
    net->xw_cap = 0;
    hipError_t e = hipMalloc((void **)&net->xw, sizeof(float) * anet::kTnXPad * (size_t)batch);
    if (e != hipSuccess) return fail(ctx, ANET_ERR_NOMEM, std::string("hipMalloc(timenet workspace): ") + hipGetErrorString(e));
    net->xw_cap = batch;
  }
  hipLaunchKernelGGL(anet::k_timenet_encode<L>, dim3((unsigned)batch), dim3(256), 0, st, net->w, state, hpolys, batch, skip, net->xw);
  ANET_HIP(ctx, hipGetLastError());
  constexpr size_t lds = sizeof(float) * anet::tn_tile_lds<L>();
  ANET_HIP(ctx, hipFuncSetAttribute((const void *)anet::k_timenet_tile<L>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const unsigned tiles = (unsigned)((batch + anet::kTnTile - 1) / anet::kTnTile);
  hipLaunchKernelGGL(anet::k_timenet_tile<L>, dim3(tiles), dim3(256), lds, st, net->w, (const float *)net->xw, batch, out);
  ANET_HIP(ctx, hipGetLastError());
  return ANET_OK;
}

}  // namespace

extern "C" {

int anet_timenet_create(anet_ctx *ctx, int seq_len, int hidden, const float *const *weights, anet_timenet **out) {
  ANET_ON_DEVICE(ctx);
  if (!out) return fail(ctx, ANET_ERR_INVALID, "anet_timenet_create: out is NULL");
  *out = nullptr;
  if (seq_len != 5 && seq_len != 10) return fail(ctx, ANET_ERR_UNSUPPORTED, "anet_timenet_create: seq_len must be 5 or 10");
  if (hidden != anet::kTnHidden) return fail(ctx, ANET_ERR_UNSUPPORTED, "anet_timenet_create: hidden must be 256");
  if (!weights) return fail(ctx, ANET_ERR_INVALID, "anet_timenet_create: weights is NULL");
  for (int i = 0; i < N_TENSORS; ++i)
    if (!weights[i]) return fail(ctx, ANET_ERR_INVALID, "anet_timenet_create: a weight tensor is NULL");
  const int H = anet::kTnHidden, flat = 16 * (seq_len / 4);
  const size_t n[N_TENSORS] = {8 * 9 * 3, 8, 6 * 8, 6, 16 * 50 * 9, 16, (size_t)32 * flat, 32, (size_t)4 * H * anet::kTnX,
                               (size_t)4 * H * H, (size_t)4 * H, (size_t)4 * H, (size_t)H, 1, (size_t)H, 1};
  // device image: SC_W .. HF_B, T_W, S_W (each padded to 4 floats), then the packed operand (16-byte aligned)
  const int small[] = {SC_W, SC_B, SF_W, SF_B, HC_W, HC_B, HF_W, HF_B, T_W, S_W};
  size_t off[N_TENSORS] = {0}, total = 0;
  for (int i : small) {
    off[i] = total;
    total += (n[i] + 3) / 4 * 4;
  }
  const size_t packed_off = total;
  total += (size_t)anet::kTnPackedFloats;
  std::vector<float> img(total, 0.0f);
  for (int i : small) memcpy(img.data() + off[i], weights[i], sizeof(float) * n[i]);
  float *pk = img.data() + packed_off;
  for (int u = 0; u < H; ++u)
    for (int k = 0; k < H + anet::kTnXPad; ++k)
      for (int g = 0; g < 4; ++g) {
        const size_t row = (size_t)g * H + u;
        float v = 0.0f;
        if (k < H) v = weights[W_HH][row * H + k];
        else if (k - H < anet::kTnX) v = weights[W_IH][row * anet::kTnX + (k - H)];
        else if (k - H == anet::kTnX) v = weights[B_IH][row] + weights[B_HH][row];
        pk[anet::timenet_pack_index(u, k) * 4 + g] = v;
      }
  anet_timenet *net = new anet_timenet;
  net->ctx = ctx;
  net->device = ctx->device;
  net->seq_len = seq_len;
  net->weight_bytes = sizeof(float) * total;
  hipError_t e = hipMalloc((void **)&net->d_weights, net->weight_bytes);
  if (e != hipSuccess) {
    delete net;
    return fail(ctx, ANET_ERR_NOMEM, std::string("hipMalloc(timenet weights): ") + hipGetErrorString(e));
  }
  e = hipMemcpy(net->d_weights, img.data(), net->weight_bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(net->d_weights);
    delete net;
    return hip_fail(ctx, e, "hipMemcpy(timenet weights)");
  }
  const float *d = net->d_weights;
  net->w = anet::TimeNetWeights{d + off[SC_W], d + off[SC_B], d + off[SF_W], d + off[SF_B], d + off[HC_W], d + off[HC_B],
                                d + off[HF_W], d + off[HF_B], d + off[T_W],  d + off[S_W],  weights[T_B][0], weights[S_B][0],
                                (const float4 *)(d + packed_off)};
  *out = net;
  return ANET_OK;
}

void anet_timenet_destroy(anet_timenet *net) {
  if (!net) return;
  DeviceGuard guard;
  int cur = -1;
  if (hipGetDevice(&cur) == hipSuccess && cur != net->device && hipSetDevice(net->device) == hipSuccess)
    guard.prev = cur;
  if (net->d_weights) (void)hipFree(net->d_weights);
  if (net->xw) (void)hipFree(net->xw);
  if (net->stage) (void)hipFree(net->stage);
  delete net;
}

int64_t anet_timenet_device_bytes(const anet_timenet *net) {
  if (!net) return 0;
  return (int64_t)(net->weight_bytes + sizeof(float) * anet::kTnXPad * (size_t)net->xw_cap + net->stage_bytes);
}

int anet_timenet_forward_dev(anet_ctx *ctx, anet_timenet *net, int seq_len, int64_t batch, const float *state, const float *hpolys,
                             double threshold, int flags, float *times, float *tf, float *stop, int32_t *count, void *stream) {
  ANET_ON_DEVICE(ctx);
  int rc = check_forward(ctx, net, seq_len, batch, flags);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!state || !hpolys || !times || !count) return fail(ctx, ANET_ERR_INVALID, "anet_timenet_forward_dev: NULL pointer");
  const anet::TimeNetOut out{times, tf, stop, count, threshold};
  hipStream_t st = (hipStream_t)stream;
  return seq_len == 5 ? launch<5>(ctx, net, batch, state, hpolys, flags, out, st)
                      : launch<10>(ctx, net, batch, state, hpolys, flags, out, st);
}

int anet_timenet_forward(anet_ctx *ctx, anet_timenet *net, int seq_len, int64_t batch, const float *state, const float *hpolys,
                         double threshold, int flags, float *times, float *tf, float *stop, int32_t *count) {
  ANET_ON_DEVICE(ctx);
  int rc = check_forward(ctx, net, seq_len, batch, flags);
  if (rc) return rc;
  if (batch == 0) return ANET_OK;
  if (!state || !hpolys || !times || !count) return fail(ctx, ANET_ERR_INVALID, "anet_timenet_forward: NULL pointer");
  const size_t L = (size_t)seq_len, nb = (size_t)batch, n_state = nb * 18, n_hp = nb * anet::kTnRows * 4 * L, n_out = nb * L;
  float *d_state, *d_hp, *d_times, *d_tf, *d_stop;
  int32_t *d_count;
  auto layout = [&](void *w) {
    anet::Cursor c(w);
    d_state = c.take<float>(n_state); d_hp = c.take<float>(n_hp); d_times = c.take<float>(n_out); d_tf = c.take<float>(n_out);
    d_stop = c.take<float>(n_out); d_count = c.take<int32_t>(nb);
    return (size_t)c.bytes;
  };
  const size_t need = layout(nullptr);
  if (need > net->stage_bytes) {
    if (net->stage) ANET_HIP(ctx, hipFree(net->stage));
    net->stage = nullptr;
    net->stage_bytes = 0;
    hipError_t e = hipMalloc(&net->stage, need);
    if (e != hipSuccess) return fail(ctx, ANET_ERR_NOMEM, std::string("hipMalloc(timenet staging): ") + hipGetErrorString(e));
    net->stage_bytes = need;
  }
  (void)layout(net->stage);
  ANET_HIP(ctx, hipMemcpyAsync(d_state, state, sizeof(float) * n_state, hipMemcpyHostToDevice, ctx->stream));
  ANET_HIP(ctx, hipMemcpyAsync(d_hp, hpolys, sizeof(float) * n_hp, hipMemcpyHostToDevice, ctx->stream));
  rc = anet_timenet_forward_dev(ctx, net, seq_len, batch, d_state, d_hp, threshold, flags, d_times, tf ? d_tf : nullptr,
                                stop ? d_stop : nullptr, d_count, ctx->stream);
  if (rc) return rc;
  ANET_HIP(ctx, hipMemcpyAsync(times, d_times, sizeof(float) * n_out, hipMemcpyDeviceToHost, ctx->stream));
  if (tf) ANET_HIP(ctx, hipMemcpyAsync(tf, d_tf, sizeof(float) * n_out, hipMemcpyDeviceToHost, ctx->stream));
  if (stop) ANET_HIP(ctx, hipMemcpyAsync(stop, d_stop, sizeof(float) * n_out, hipMemcpyDeviceToHost, ctx->stream));
  ANET_HIP(ctx, hipMemcpyAsync(count, d_count, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, ctx->stream));
  ANET_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ANET_OK;
}

}  // extern "C"
