// The time-allocation network (minsnap_network_conv_lstm.py:37-88, 114-187) as three kernels, all arithmetic in float32:
//
//   state  (9, 2)     -> Conv1d(9->8, k 3, pad 1) -> ReLU -> MaxPool1d(2) -> Linear(8->6)
//   hpolys (50, 4, L) -> Conv2d(50->16, 3x3, pad 1) -> ReLU -> MaxPool2d(2) -> MaxPool2d(2) -> Flatten -> Linear(->32)
//   x = [6 | 32], the same at every step;  h = c = 0;  L steps of an LSTM cell, hidden 256, gate order i, f, g, o;
//   tf_k = w_t . h + b_t,  stop_k = sigmoid(w_s . h + b_s);  count = 1 + first k with stop_k > threshold (L if none);
//   times = tf[:count], zero after.
//
//   k_timenet_encode  one workgroup per problem: both encoders, x (38 values, then a 1 for the bias row and a 0) to the workspace.
//   k_timenet_tile    one workgroup per 32 problems, persistent over the L steps.  The 1024 gate pre-activations of the tile are
//                     32 accumulators of v_mfma_f32_32x32x2_f32 (problems x units, one per gate and 32-unit slice): a lane holds
//                     i, f, g, o of ONE unit for 16 problems, so the nonlinearities and the c, h update run on the accumulators
//                     and the gate vector is never stored.  h of the tile lives in LDS, k-major (the A operand of a k-step is 64
//                     consecutive floats), in two buffers; c and the input's share of the gates (computed once, by the same
//                     instruction over x) live in registers.
//   k_timenet_single  one workgroup per problem, a thread per hidden unit, encoders fused in: the planner's call (batch 1).
//
// W_hh, W_ih and b_ih + b_hh are repacked once (timenet_pack_index) into the order both recurrent kernels read: per 32-unit slice
// and k-pair, 64 lanes x 4 gates, so a wave's B operands for the four gates of a k-step are one 16-byte load per lane.
// The two pools of the hpolys encoder keep conv outputs at rows 0..3, columns 0..4 (L / 4) - 1 only; nothing else is computed.
// sigmoid is 1 / (1 + expf(-x)) with the accurate expf; tanh is tanhf.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace anet {

constexpr int kTnHidden = 256;            // LSTM hidden size the kernels are written for
constexpr int kTnRows = 50;               // rows of a polytope = input channels of the Conv2d
constexpr int kTnX = 38;                  // 6 + 32
constexpr int kTnXPad = 40;               // x, 1 (multiplies the bias row), 0
constexpr int kTnTile = 32;               // problems per workgroup of k_timenet_tile: the M of the 32x32x2 instruction
constexpr int kTnKPairs = (kTnHidden + kTnXPad) / 2;   // k-steps of the packed operand: 128 of W_hh, then 20 of [W_ih | bias | 0]
constexpr int kTnSlices = kTnHidden / 32;
constexpr int kTnMaxL = 10;
constexpr int64_t kTnPackedFloats = (int64_t)kTnSlices * kTnKPairs * 64 * 4;

// float4 index of (unit u, k) in the packed operand; component = gate.  k < 256: W_hh[g * 256 + u][k]; 256 <= k < 294:
// W_ih[g * 256 + u][k - 256]; k = 294: b_ih + b_hh; k = 295: 0.
__host__ __device__ inline int64_t timenet_pack_index(int u, int k) {
  return ((int64_t)(u >> 5) * kTnKPairs + (k >> 1)) * 64 + (k & 1) * 32 + (u & 31);
}

struct TimeNetWeights {  // device pointers into the handle's one allocation
  const float *sc_w, *sc_b, *sf_w, *sf_b;  // state encoder: conv (8, 9, 3), (8); linear (6, 8), (6)
  const float *hc_w, *hc_b, *hf_w, *hf_b;  // hpolys encoder: conv (16, 50, 3, 3), (16); linear (32, 16 (L / 4)), (32)
  const float *w_t, *w_s;                  // heads (256) each
  float b_t, b_s;
  const float4 *packed;
};

struct TimeNetOut {  // times [B][L], count [B]; tf, stop [B][L] or nullptr
  float *times, *tf, *stop;
  int32_t *count;
  double threshold;
};

typedef float tn_f32x16 __attribute__((ext_vector_type(16)));

__device__ inline float tn_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// floats of LDS tn_encode needs
template <int L>
constexpr int tn_encode_lds() {
  return kTnRows * 6 * (L + 2) + 16 * 4 * (4 * (L / 4)) + 32 + 8 + 2;
}

// Both encoders of one problem by a workgroup of 256 threads; x[0..39] (LDS) is complete after the closing barrier.
// skip: channels (polytope rows) after the last non-zero one and taps on columns (polytopes) after the last non-zero one are
// left out; each is a product with an exact zero, the order of the rest is unchanged.
template <int L>
__device__ inline void tn_encode(const TimeNetWeights &w, const float *__restrict__ state, const float *__restrict__ hp, bool skip,
                                 float *sm, float *x) {
  constexpr int PW = L + 2, CW = 4 * (L / 4), NQ = L / 4, NIN = kTnRows * 6 * PW;
  float *in = sm, *conv = in + NIN, *feat = conv + 16 * 4 * CW, *spool = feat + 32;
  int *ext = (int *)(spool + 8);  // [0]: channels in use, [1]: columns in use
  const int tid = threadIdx.x;
  if (tid < 2) ext[tid] = 0;
  __syncthreads();
  for (int i = tid; i < NIN; i += 256) {
    const int c = i / (6 * PW), yy = (i / PW) % 6, xx = i % PW;
    float v = 0.0f;
    if (yy >= 1 && yy <= 4 && xx >= 1 && xx <= L) {
      v = hp[(c * 4 + (yy - 1)) * L + (xx - 1)];
      if (v != 0.0f) {
        atomicMax(&ext[0], c + 1);
        atomicMax(&ext[1], xx);
      }
    }
    in[i] = v;
  }
  __syncthreads();
  const int nch = skip ? ext[0] : kTnRows, ncol = skip ? ext[1] : L;
  for (int o = tid; o < 16 * 4 * CW; o += 256) {
    const int ch = o / (4 * CW), y = (o / CW) % 4, xo = o % CW;
    // input column of tap dx is xo + dx - 1: taps with xo + dx - 1 >= ncol read padding
    int ndx = ncol - xo + 1;
    ndx = ndx > 3 ? 3 : ndx;
    float acc = w.hc_b[ch];
    const float *wk = w.hc_w + (size_t)ch * kTnRows * 9;
    for (int c = 0; c < nch; ++c) {
      const float *ip = in + (c * 6 + y) * PW + xo;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
        for (int dx = 0; dx < ndx; ++dx) acc = fmaf(ip[dy * PW + dx], wk[c * 9 + dy * 3 + dx], acc);
    }
    conv[o] = fmaxf(acc, 0.0f);
  }
  if (tid >= 64 && tid < 72) {  // state encoder, a thread per channel: out[t] = b + sum_{c, k} w[c][k] in[c][t + k - 1]
    const int ch = tid - 64;
    float p0 = w.sc_b[ch], p1 = p0;
    for (int c = 0; c < 9; ++c) {
      const float s0 = state[2 * c], s1 = state[2 * c + 1];
      const float *wk = w.sc_w + (ch * 9 + c) * 3;
      p0 = fmaf(s1, wk[2], fmaf(s0, wk[1], p0));
      p1 = fmaf(s1, wk[1], fmaf(s0, wk[0], p1));
    }
    spool[ch] = fmaxf(fmaxf(p0, 0.0f), fmaxf(p1, 0.0f));
  }
  __syncthreads();
  if (tid < 16 * NQ) {  // the two 2x2 pools: the maximum over rows 0..3, columns 4 q .. 4 q + 3
    const int ch = tid / NQ, q = tid % NQ;
    float m = conv[(ch * 4) * CW + 4 * q];
    for (int y = 0; y < 4; ++y)
      for (int xq = 0; xq < 4; ++xq) m = fmaxf(m, conv[(ch * 4 + y) * CW + 4 * q + xq]);
    feat[tid] = m;  // channel-major flatten: index ch * (L / 4) + q
  }
  __syncthreads();
  if (tid < 32) {
    float a = w.hf_b[tid];
    for (int f = 0; f < 16 * NQ; ++f) a = fmaf(feat[f], w.hf_w[tid * 16 * NQ + f], a);
    x[6 + tid] = a;
  } else if (tid >= 64 && tid < 70) {
    const int j = tid - 64;
    float a = w.sf_b[j];
    for (int q = 0; q < 8; ++q) a = fmaf(spool[q], w.sf_w[j * 8 + q], a);
    x[j] = a;
  } else if (tid == 70) {
    x[kTnX] = 1.0f;
  } else if (tid == 71) {
    x[kTnX + 1] = 0.0f;
  }
  __syncthreads();
}

// count and the zero-padded times of one problem from its L steps (tfv, stv: stride `st` floats), written with tf and stop
template <int L>
__device__ inline void tn_finish(const TimeNetOut &o, int64_t b, const float *tfv, const float *stv, int st) {
  int cnt = L;
  for (int k = L - 1; k >= 0; --k)
    if ((double)stv[k * st] > o.threshold) cnt = k + 1;
  o.count[b] = cnt;
  for (int k = 0; k < L; ++k) {
    o.times[b * L + k] = k < cnt ? tfv[k * st] : 0.0f;
    if (o.tf) o.tf[b * L + k] = tfv[k * st];
    if (o.stop) o.stop[b * L + k] = stv[k * st];
  }
}

template <int L>
__global__ __launch_bounds__(256) void k_timenet_encode(TimeNetWeights w, const float *__restrict__ state,
                                                        const float *__restrict__ hpolys, int64_t B, int skip,
                                                        float *__restrict__ xw) {
  __shared__ float sm[tn_encode_lds<L>()];
  __shared__ float x[kTnXPad];
  const int64_t b = blockIdx.x;
  if (b >= B) return;
  tn_encode<L>(w, state + b * 18, hpolys + b * (kTnRows * 4 * L), skip != 0, sm, x);
  if (threadIdx.x < kTnXPad) xw[b * kTnXPad + threadIdx.x] = x[threadIdx.x];
}

template <int L>
__global__ __launch_bounds__(256) void k_timenet_single(TimeNetWeights w, const float *__restrict__ state,
                                                        const float *__restrict__ hpolys, int64_t B, int skip, TimeNetOut out) {
  __shared__ float sm[tn_encode_lds<L>()];
  __shared__ float x[kTnXPad];
  __shared__ float hs[2][kTnHidden];
  __shared__ float red[2][2][4];  // by step parity
  __shared__ float tfv[L], stv[L];
  const int64_t b = blockIdx.x;
  if (b >= B) return;
  tn_encode<L>(w, state + b * 18, hpolys + b * (kTnRows * 4 * L), skip != 0, sm, x);
  const int j = threadIdx.x;  // hidden unit
  const float4 *wp = w.packed;
  float gx0 = 0.0f, gx1 = 0.0f, gx2 = 0.0f, gx3 = 0.0f;
  for (int k = 0; k < kTnXPad; ++k) {
    const float4 v = wp[timenet_pack_index(j, kTnHidden + k)];
    const float xk = x[k];
    gx0 = fmaf(xk, v.x, gx0); gx1 = fmaf(xk, v.y, gx1); gx2 = fmaf(xk, v.z, gx2); gx3 = fmaf(xk, v.w, gx3);
  }
  const float wt = w.w_t[j], ws = w.w_s[j];
  float c = 0.0f;
  hs[0][j] = 0.0f;
  __syncthreads();
  for (int step = 0; step < L; ++step) {
    const float *hc = hs[step & 1];
    float a0 = gx0, a1 = gx1, a2 = gx2, a3 = gx3;
    if (step > 0) {  // h = 0 at the first step
#pragma unroll 8
      for (int k = 0; k < kTnHidden; ++k) {
        const float4 v = wp[timenet_pack_index(j, k)];
        const float hk = hc[k];
        a0 = fmaf(hk, v.x, a0); a1 = fmaf(hk, v.y, a1); a2 = fmaf(hk, v.z, a2); a3 = fmaf(hk, v.w, a3);
      }
    }
    c = tn_sigmoid(a1) * c + tn_sigmoid(a0) * tanhf(a2);
    const float h = tn_sigmoid(a3) * tanhf(c);
    hs[(step + 1) & 1][j] = h;
    float pt = h * wt, ps = h * ws;
    for (int d = 32; d > 0; d >>= 1) {
      pt += __shfl_down(pt, d, 64);
      ps += __shfl_down(ps, d, 64);
    }
    if ((j & 63) == 0) {
      red[step & 1][0][j >> 6] = pt;
      red[step & 1][1][j >> 6] = ps;
    }
    __syncthreads();
    if (j == 0) {
      const float(*rd)[4] = red[step & 1];
      tfv[step] = w.b_t + (((rd[0][0] + rd[0][1]) + rd[0][2]) + rd[0][3]);
      stv[step] = tn_sigmoid(w.b_s + (((rd[1][0] + rd[1][1]) + rd[1][2]) + rd[1][3]));
    }
    // this parity of red is rewritten two steps on, past the next step's barrier, which thread 0 reaches after reading it
  }
  __syncthreads();
  if (j == 0) tn_finish<L>(out, b, tfv, stv, 1);
}

// LDS of k_timenet_tile in floats: h (two buffers, k-major [256][32]), x ([40][32]), head partials [2][4][32], tf and stop
// of the tile [L][32] each
template <int L>
constexpr int tn_tile_lds() {
  return 2 * kTnHidden * kTnTile + kTnXPad * kTnTile + 2 * 4 * kTnTile + 2 * L * kTnTile;
}

template <int L>
__global__ __launch_bounds__(256) void k_timenet_tile(TimeNetWeights w, const float *__restrict__ xw, int64_t B, TimeNetOut out) {
  extern __shared__ __attribute__((aligned(16))) float tn_lds[];
  float *hb0 = tn_lds, *hb1 = hb0 + kTnHidden * kTnTile, *xs = hb1 + kTnHidden * kTnTile, *part = xs + kTnXPad * kTnTile,
        *tfv = part + 2 * 4 * kTnTile, *stv = tfv + L * kTnTile;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b0 = (int64_t)blockIdx.x * kTnTile;
  for (int i = tid; i < kTnXPad * kTnTile; i += 256) {  // xs[k][p]; problems past the batch compute on zeros and write nothing
    const int k = i / kTnTile, p = i % kTnTile;
    xs[i] = b0 + p < B ? xw[(b0 + p) * kTnXPad + k] : 0.0f;
  }
  __syncthreads();
  // the wave's two slices of 32 units; acc/gx/c element r of a lane: unit 32 s + (lane & 31), problem row(r)
  const float4 *wp0 = w.packed + ((int64_t)(2 * wave) * kTnKPairs) * 64 + lane;
  const float4 *wp1 = wp0 + (int64_t)kTnKPairs * 64;
  tn_f32x16 gx[2][4], cst[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const float4 *wp = s ? wp1 : wp0;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int r = 0; r < 16; ++r) gx[s][g][r] = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) cst[s][r] = 0.0f;
#pragma unroll 4
    for (int kk = 0; kk < kTnXPad / 2; ++kk) {
      const float a = xs[kk * 64 + lane];
      const float4 v = wp[(kTnHidden / 2 + kk) * 64];
      gx[s][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, v.x, gx[s][0], 0, 0, 0);
      gx[s][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, v.y, gx[s][1], 0, 0, 0);
      gx[s][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, v.z, gx[s][2], 0, 0, 0);
      gx[s][3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, v.w, gx[s][3], 0, 0, 0);
    }
  }
  const int hp = tid & 31, hh = (tid >> 5) & 1, hq = tid >> 6;  // heads: problem, head, quarter of the 256-long dot
  const float *hw = hh ? w.w_s : w.w_t;
  for (int step = 0; step < L; ++step) {
    const float *hc = (step & 1) ? hb1 : hb0;
    float *hn = (step & 1) ? hb0 : hb1;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const float4 *wp = s ? wp1 : wp0;
      tn_f32x16 a0 = gx[s][0], a1 = gx[s][1], a2 = gx[s][2], a3 = gx[s][3];
      if (step > 0) {  // h = 0 at the first step
#pragma unroll 8
        for (int kk = 0; kk < kTnHidden / 2; ++kk) {
          const float a = hc[kk * 64 + lane];
          const float4 v = wp[kk * 64];
          a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, v.x, a0, 0, 0, 0);
          a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, v.y, a1, 0, 0, 0);
          a2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, v.z, a2, 0, 0, 0);
          a3 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, v.w, a3, 0, 0, 0);
        }
      }
      const int u = 32 * (2 * wave + s) + (lane & 31);
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        float4 hv;
        float *hvp = (float *)&hv;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = rg * 4 + q;
          const float cc = tn_sigmoid(a1[r]) * cst[s][r] + tn_sigmoid(a0[r]) * tanhf(a2[r]);
          cst[s][r] = cc;
          hvp[q] = tn_sigmoid(a3[r]) * tanhf(cc);
        }
        // rows 8 rg + 4 (lane >> 5) + 0..3 of column u
        *(float4 *)(hn + u * kTnTile + 8 * rg + 4 * (lane >> 5)) = hv;
      }
    }
    __syncthreads();  // the new h is complete; the old one is not read again
    {
      float a = 0.0f;
      for (int k = 64 * hq; k < 64 * hq + 64; ++k) a = fmaf(hn[k * kTnTile + hp], hw[k], a);
      part[(hh * 4 + hq) * kTnTile + hp] = a;
    }
    __syncthreads();
    if (tid < 64) {
      const float *pp = part + hh * 4 * kTnTile + hp;
      const float v = (hh ? w.b_s : w.b_t) + (((pp[0] + pp[kTnTile]) + pp[2 * kTnTile]) + pp[3 * kTnTile]);
      if (hh) stv[step * kTnTile + hp] = tn_sigmoid(v);
      else tfv[step * kTnTile + hp] = v;
    }
    // part is rewritten after the next step's first barrier only, which wave 0 reaches after reading it
  }
  __syncthreads();
  if (tid < kTnTile && b0 + tid < B) tn_finish<L>(out, b0 + tid, tfv + tid, stv + tid, kTnTile);
}

}  // namespace anet
