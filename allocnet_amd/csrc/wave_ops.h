// Wave-wide reductions of gfx950 on the DPP path (shared by the L-BFGS kernels, the one-launch MINCO evaluation
// and the interior-point QP).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace anet {

// Wave-wide reductions on the DPP path: in-row inclusive scan by row_shr 1/2/4/8, row_bcast:15 /
// row_bcast:31 to chain the four rows, total read from lane 63 as a wave-uniform scalar.  About 20 VALU
// ops, where the ds_bpermute butterfly of __shfl_xor costs several hundred cycles per reduction --
// the two-loop recursion is a chain of 2*mem_size dependent reductions.  All 64 lanes must be active.
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ double dpp_f64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xf, true);  // masked rows / missing sources read 0
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xf, true);
  return __hiloint2double(hi, lo);
}
template <int LANE = 63>
__device__ __forceinline__ double last_lane(double v) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), LANE),
                          __builtin_amdgcn_readlane(__double2loint(v), LANE));
}
// LAST = 15 / 31: the caller guarantees zeros in the lanes above it, so the steps that chain the upper rows would only
// add zeros and are left out (the value is the same; a problem of nine variables saves a third of every reduction).
template <int LAST = 63>
__device__ __forceinline__ double wave_sum(double v) {
  v += dpp_f64<0x111>(v);
  v += dpp_f64<0x112>(v);
  v += dpp_f64<0x114>(v);
  v += dpp_f64<0x118>(v);
  if constexpr (LAST >= 31) v += dpp_f64<0x142, 0xa>(v);
  if constexpr (LAST >= 63) v += dpp_f64<0x143, 0xc>(v);
  return last_lane<LAST>(v);
}
// maximum of NON-NEGATIVE values (0 is the fill of masked / missing lanes)
template <int LAST = 63>
__device__ __forceinline__ double wave_max_nonneg(double v) {
  v = fmax(v, dpp_f64<0x111>(v));
  v = fmax(v, dpp_f64<0x112>(v));
  v = fmax(v, dpp_f64<0x114>(v));
  v = fmax(v, dpp_f64<0x118>(v));
  if constexpr (LAST >= 31) v = fmax(v, dpp_f64<0x142, 0xa>(v));
  if constexpr (LAST >= 63) v = fmax(v, dpp_f64<0x143, 0xc>(v));
  return last_lane<LAST>(v);
}

// minimum over the wave; lanes without a source keep their own value (bound_ctrl off, old = the value itself)
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ double dpp_keep_f64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_min_f64(double v) {
  v = fmin(v, dpp_keep_f64<0x111>(v));
  v = fmin(v, dpp_keep_f64<0x112>(v));
  v = fmin(v, dpp_keep_f64<0x114>(v));
  v = fmin(v, dpp_keep_f64<0x118>(v));
  v = fmin(v, dpp_keep_f64<0x142, 0xa>(v));
  v = fmin(v, dpp_keep_f64<0x143, 0xc>(v));
  return last_lane<63>(v);
}

// a value every lane holds identically (loaded from a wave-uniform address) -> SGPR pair
__device__ __forceinline__ double uniform_f64(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                          __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
// Two problems per wave (32 lanes each): the same scans, chained over the two rows of a half only; each half then
// reads its total from its own last lane.  Needs the lanes of a HALF to be active together, not the whole wave.
__device__ __forceinline__ double half_pick(double v) {
  const double lo = last_lane<31>(v), hi = last_lane<63>(v);
  return (threadIdx.x & 32) ? hi : lo;
}
__device__ __forceinline__ double half_sum(double v) {
  v += dpp_f64<0x111>(v);
  v += dpp_f64<0x112>(v);
  v += dpp_f64<0x114>(v);
  v += dpp_f64<0x118>(v);
  v += dpp_f64<0x142, 0xa>(v);
  return half_pick(v);
}
__device__ __forceinline__ double half_max_nonneg(double v) {
  v = fmax(v, dpp_f64<0x111>(v));
  v = fmax(v, dpp_f64<0x112>(v));
  v = fmax(v, dpp_f64<0x114>(v));
  v = fmax(v, dpp_f64<0x118>(v));
  v = fmax(v, dpp_f64<0x142, 0xa>(v));
  return half_pick(v);
}

template <int CTRL>
__device__ __forceinline__ double dpp_add(double v) { return v + dpp_f64<CTRL>(v); }
// the lanes 2k, 2k+1 as a pair (quad_perm [1,0,3,2]): the other lane's value, and the sum of both
__device__ __forceinline__ double lane_pair_swap(double v) { return dpp_f64<0xB1>(v); }
__device__ __forceinline__ double pair_sum(double v) { return dpp_add<0xB1>(v); }
// sum over the G adjacent lanes of a group (G = 4, 8, 16; every lane of the group ends with the total)
template <int G>
__device__ __forceinline__ double group_sum(double v) {
  v = dpp_add<0xB1>(v);                          // quad_perm [1,0,3,2]
  v = dpp_add<0x4E>(v);                          // quad_perm [2,3,0,1]
  if constexpr (G >= 8) v = dpp_add<0x141>(v);   // row_half_mirror
  if constexpr (G >= 16) v = dpp_add<0x140>(v);  // row_mirror
  return v;
}

}  // namespace anet
