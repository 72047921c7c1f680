// tpe_wave.hpp -- wave and block primitives shared by the TPE kernels.
//
// Wave64 everywhere: 64-lane butterflies and scans, block sizes multiples of
// 64.  Names are <scope>_<what>: scope wave (64 lanes), row (a 16-lane DPP
// row) or block; reductions (max / sum / min: every lane or thread gets the
// result), inclusive scans in lane or thread order (prefix_* from the front,
// suffix_* from the back), block_excl_sum, and the *_prefix_count searches.
// Block primitives take their LDS scratch (one entry per wave) and sync.
// (Moved as they were; the never-called wave_sum_f/d/dpp, wave_max_d, dpp_f dropped.)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tpe {

constexpr int kWave = 64;

__device__ __forceinline__ int lane_id() { return threadIdx.x & (kWave - 1); }

// wave reductions (shuffle butterflies)
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, kWave));
  return v;
}
// (wave-uniform results, in a scalar register)
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = min(v, __shfl_xor(v, off, kWave));
  return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = max(v, __shfl_xor(v, off, kWave));
  return __builtin_amdgcn_readfirstlane(v);
}

// DPP moves (all 64 lanes active): exchanges without the LDS crossbar
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)u, CTRL, 0xF, 0xF, true);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)(u >> 32), CTRL, 0xF, 0xF,
                                                         true);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
// lanes whose source is outside the wave keep `old` (a scan's identity)
template <int CTRL, int ROWM>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t old, uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, ROWM, 0xF, false);
}
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141, kDppMirror = 0x140;
__device__ __forceinline__ int row_max_i(int v) {  // max over the lane's 16-lane DPP row
  v = max(v, __builtin_amdgcn_mov_dpp(v, kDppXor1, 0xF, 0xF, true));
  v = max(v, __builtin_amdgcn_mov_dpp(v, kDppXor2, 0xF, 0xF, true));
  v = max(v, __builtin_amdgcn_mov_dpp(v, kDppHalfMirror, 0xF, 0xF, true));
  v = max(v, __builtin_amdgcn_mov_dpp(v, kDppMirror, 0xF, 0xF, true));
  return v;
}
// inclusive wave scan by DPP (row shifts, then the row broadcasts of 15 and 31)
template <int CTRL, int ROWM>
__device__ __forceinline__ void scan_step_u64(uint64_t& v) {
  const uint32_t lo = dpp_u32<CTRL, ROWM>(0u, (uint32_t)v);
  const uint32_t hi = dpp_u32<CTRL, ROWM>(0u, (uint32_t)(v >> 32));
  v += ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t wave_prefix_sum_u64(uint64_t v) {
  scan_step_u64<0x111, 0xF>(v);  // row_shr:1
  scan_step_u64<0x112, 0xF>(v);  // row_shr:2
  scan_step_u64<0x114, 0xF>(v);  // row_shr:4
  scan_step_u64<0x118, 0xF>(v);  // row_shr:8
  scan_step_u64<0x142, 0xA>(v);  // row_bcast:15 -> rows 1, 3
  scan_step_u64<0x143, 0xC>(v);  // row_bcast:31 -> rows 2, 3
  return v;
}

// 64-bit lane exchanges as two 32-bit ones: lane l's value in every lane
// (l wave-uniform), and the butterfly partner's
__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, int l) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l) << 32) |
         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
}
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int o) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, kWave);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, kWave);
  return ((uint64_t)hi << 32) | lo;
}

// block reductions; result valid in every thread.  `sh` holds >= BS / 64 T.
template <int BS, typename T>
__device__ __forceinline__ T block_sum(T v, T* sh) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  __syncthreads();
  if (lane == 0) sh[wid] = v;
  __syncthreads();
  T r = sh[0];
#pragma unroll
  for (int k = 1; k < BS / kWave; ++k) r += sh[k];
  return r;
}

template <int BS, typename T>
__device__ __forceinline__ T block_max(T v, T* sh) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, kWave));
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  __syncthreads();
  if (lane == 0) sh[wid] = v;
  __syncthreads();
  T r = sh[0];
#pragma unroll
  for (int k = 1; k < BS / kWave; ++k) r = fmax(r, sh[k]);
  return r;
}

// inclusive block scans over the threads' values in thread order: wave
// shuffles, then the waves' totals through LDS (`sh`: one entry per wave).
// Every thread gets its own inclusive result.
__device__ __forceinline__ double block_prefix_max(double v, double* sh) {
  const int lane = lane_id(), wid = threadIdx.x / kWave;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const double o = __shfl_up(v, off, kWave);
    if (lane >= off) v = fmax(v, o);
  }
  __syncthreads();
  if (lane == kWave - 1) sh[wid] = v;
  __syncthreads();
  for (int w = 0; w < wid; ++w) v = fmax(v, sh[w]);
  return v;
}
__device__ __forceinline__ int block_prefix_sum(int v, int* sh) {
  const int lane = lane_id(), wid = threadIdx.x / kWave;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int o = __shfl_up(v, off, kWave);
    if (lane >= off) v += o;
  }
  __syncthreads();
  if (lane == kWave - 1) sh[wid] = v;
  __syncthreads();
  for (int w = 0; w < wid; ++w) v += sh[w];
  return v;
}
template <int BS>  // min from the back
__device__ __forceinline__ double block_suffix_min(double v, double* sh) {
  const int lane = lane_id(), wid = threadIdx.x / kWave;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const double u = __shfl_down(v, o, kWave);
    if (lane + o < kWave) v = fmin(v, u);
  }
  __syncthreads();
  if (lane == 0) sh[wid] = v;
  __syncthreads();
  for (int w = wid + 1; w < BS / kWave; ++w) v = fmin(v, sh[w]);
  return v;
}

// exclusive block scan of one int per thread (sh reusable after the call);
// total: the block's sum
template <int BS>
__device__ __forceinline__ int block_excl_sum(int v, int* sh, int& total) {
  constexpr int kNW = BS / kWave;
  const int lane = lane_id(), wid = threadIdx.x / kWave;
  int incl = v;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int x = __shfl_up(incl, o, kWave);
    if (lane >= o) incl += x;
  }
  __syncthreads();
  if (lane == kWave - 1) sh[wid] = incl;
  __syncthreads();
  int pos = incl - v;
  total = 0;
#pragma unroll
  for (int w = 0; w < kNW; ++w) {
    pos += w < wid ? sh[w] : 0;
    total += sh[w];
  }
  __syncthreads();
  return pos;
}

// how many leading k in [0, n) satisfy pred (pred holds on a prefix): a
// wave-wide search, kWave probes per round (three rounds for n <= 2^18); call
// by the whole wave (n wave-uniform)
template <typename F>
__device__ __forceinline__ int wave_prefix_count(int n, F pred) {
  int lo = 0, len = n;
  const int t = lane_id();
  while (len > 0) {  // wave-uniform
    const int stride = (len + kWave - 1) / kWave;
    const int nprobe = (len + stride - 1) / stride;
    const int p = lo + min((t + 1) * stride, len) - 1;
    // pred holds on a prefix, so the lanes whose probe holds are a prefix too
    const int c = __popcll(__ballot(t < nprobe && pred(p)));
    if (c == nprobe) return lo + len;
    lo += c * stride;
    len = min(stride, len - c * stride) - 1;  // (probe c failed: the boundary is before it)
  }
  return lo;
}
// the same, block-wide: BS probes per round (three rounds for n <= 2^24)
template <int BS, typename F>
__device__ __forceinline__ int block_prefix_count(int n, F pred) {
  int lo = 0, len = n;
  while (len > 0) {  // block-uniform
    const int stride = (len + BS - 1) / BS;
    const int nprobe = (len + stride - 1) / stride;
    const int t = threadIdx.x;
    const int p = lo + min((t + 1) * stride, len) - 1;
    const int c = __syncthreads_count(t < nprobe && pred(p));
    if (c == nprobe) return lo + len;
    lo += c * stride;
    len = min(stride, len - c * stride) - 1;  // (probe c failed: the boundary is before it)
  }
  return lo;
}

}  // namespace tpe
