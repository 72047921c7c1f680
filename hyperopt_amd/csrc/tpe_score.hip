// tpe_score.hip -- candidate sampling, EI scoring and argmax for the
// continuous, unquantized labels: the dense and the sorted scorers.
// (Quantized labels: tpe_quantized.hip; categorical ones: tpe_categorical.hip.)
//
// Replaces, per label:
//   GMM1 / LGMM1 sampling          hyperopt/tpe.py:79-106, 229-257
//   GMM1_lpdf / LGMM1_lpdf         hyperopt/tpe.py:117-180, 265-307 (+ logsum_rows :260-262)
//   broadcast_best (argmax)        hyperopt/tpe.py:649-658
//
// Continuous, unquantized labels (the N x M hot loop):
//   grid = (candidate chunks, labels); a block owns kBS*R candidates held in
//   registers (R per thread), sampled with Philox from the below mixture (or
//   read, for injected candidates), and streams each mixture's components
//   through one LDS tile (float4 {a,b,c,-} / double4 {mu,1/sigma,logcoef,w}),
//   read back as wave-wide broadcasts.  fp32 terms are evaluated as
//       t = xc*a + b ;  v = c - t*t ;  sum += 2^v        (one v_exp_f32 / pair)
//   with the log2 coefficients pre-offset by the mixture's max, so no running
//   max is needed; a wave whose prior term shows the sum could leave the
//   normal range (v_prior < -100) takes the exact online log-sum-exp instead.
//   fp64 (parity mode) always runs the exact online log-sum-exp.
//   The argmax is fused: per-thread -> wave butterfly -> block -> partials ->
//   one reduce block per label.  Nothing per-candidate touches HBM unless the
//   caller asks for the per-candidate outputs.
//
// Exports: tpe_score_partials, tpe_score_continuous, tpe_sample,
// tpe_best_combine, tpe_sort_layout, tpe_sort_candidates, tpe_score_sorted.
#include "tpe_common.hpp"
#include "tpe_sample.hpp"

namespace tpe {
namespace {
constexpr int kR32 = 8;
constexpr int kR64 = 4;
constexpr int kTile32 = 1024;  // float4 components per tile (16 KB)
constexpr int kTile64 = 512;   // double4 components per tile (16 KB)
constexpr float kFastFloor = -100.0f;            // log2 units below the mixture max
constexpr float kLn2f = 0.6931471805599453f;

// ---------------------------------------------------------------------------
// mixture log-density at R candidates, fp32 (log2-domain, offset by cmax)
// ---------------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int R>
struct Lse32 {
  float xc[R], s[R], m[R];
  bool fast;
};

// centre the candidates and decide the wave's mode: the fast path (fixed
// offset, one v_exp_f32 per pair) is exact whenever the prior component's
// term keeps the sum in the normal fp32 range for every lane of the wave
template <int R>
__device__ __forceinline__ void lse32_begin(Lse32<R>& L, const float4* __restrict__ coef,
                                            const tpe_seg& S, const float (&y)[R]) {
  const float cen = (float)S.center;
  const float4 cp = coef[S.prior_pos];
  bool ok = true;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    L.xc[r] = y[r] - cen;
    const float t = fmaf(L.xc[r], cp.x, cp.y);
    ok = ok && (fmaf(-t, t, cp.z) >= kFastFloor);
    L.s[r] = 0.0f;
    L.m[r] = -INFINITY;
  }
  L.fast = __all(ok);
}

// accumulate the mm components staged in `tile` (block-uniform mm)
template <int R>
__device__ __forceinline__ void lse32_tile(Lse32<R>& L, const float4* tile, int mm) {
  if (L.fast) {
    // packed fp32: two candidates per v_pk_fma_f32 (the microbenchmark in
    // tools/valu_microbench.hip: 15.8 vs 18.9 cycles per 64 pairs)
    static_assert(R % 2 == 0, "R must be even");
    f32x2 xc2[R / 2], acc[R / 2];
#pragma unroll
    for (int p = 0; p < R / 2; ++p) {
      xc2[p] = f32x2{L.xc[2 * p], L.xc[2 * p + 1]};
      acc[p] = f32x2{0.0f, 0.0f};
    }
#pragma unroll 4
    for (int k = 0; k < mm; ++k) {
      const float4 c = tile[k];
      const f32x2 a2 = f32x2{c.x, c.x}, b2 = f32x2{c.y, c.y}, c2 = f32x2{c.z, c.z};
#pragma unroll
      for (int p = 0; p < R / 2; ++p) {
        const f32x2 t = __builtin_elementwise_fma(xc2[p], a2, b2);
        const f32x2 v = __builtin_elementwise_fma(-t, t, c2);
        acc[p] += f32x2{__builtin_amdgcn_exp2f(v.x), __builtin_amdgcn_exp2f(v.y)};
      }
    }
#pragma unroll
    for (int p = 0; p < R / 2; ++p) {
      L.s[2 * p] += acc[p].x;
      L.s[2 * p + 1] += acc[p].y;
    }
  } else {
    for (int k = 0; k < mm; ++k) {
      const float4 c = tile[k];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float t = fmaf(L.xc[r], c.x, c.y);
        const float v = fmaf(-t, t, c.z);
        if (v > L.m[r]) {
          L.s[r] = L.s[r] * __builtin_amdgcn_exp2f(L.m[r] - v) + 1.0f;
          L.m[r] = v;
        } else if (c.z > -INFINITY) {  // masked (wide) components add nothing
          L.s[r] += __builtin_amdgcn_exp2f(v - L.m[r]);
        }
      }
    }
  }
}

// accumulate components [k0, k1) of `coef` (block-uniform bounds; syncs)
template <int R>
__device__ __forceinline__ void lse32_accum(Lse32<R>& L, const float4* __restrict__ coef, int k0,
                                            int k1, float4* tile) {
  for (int t0 = k0; t0 < k1; t0 += kTile32) {
    const int mm = min(kTile32, k1 - t0);
    __syncthreads();
    for (int j = threadIdx.x; j < mm; j += kBS) tile[j] = coef[t0 + j];
    __syncthreads();
    lse32_tile(L, tile, mm);
  }
}

// largest / smallest term of component c over centred candidates [xlo, xhi]
// (t = xc*a + b is increasing in xc, v = c - t^2)
__device__ __forceinline__ float term_max(const float4 c, float xlo, float xhi) {
  const float tl = fmaf(xlo, c.x, c.y), th = fmaf(xhi, c.x, c.y);
  const float t2 = (tl <= 0.0f && th >= 0.0f) ? 0.0f : fminf(tl * tl, th * th);
  return c.z - t2;
}
__device__ __forceinline__ float term_min(const float4 c, float xlo, float xhi) {
  const float tl = fmaf(xlo, c.x, c.y), th = fmaf(xhi, c.x, c.y);
  return c.z - fmaxf(tl * tl, th * th);
}

// like lse32_accum, but only components whose largest term over the block's
// candidates reaches `thr` are staged (compacted, in index order) and summed.
// Returns the number of components summed (block-uniform).
template <int R>
__device__ __forceinline__ int lse32_accum_pruned(Lse32<R>& L, const float4* __restrict__ coef,
                                                  int k0, int k1, float4* tile, int* cnt,
                                                  float xlo, float xhi, float thr) {
  constexpr int kQ = kTile32 / kBS, kW = kBS / kWave;
  const int wid = threadIdx.x / kWave;
  const unsigned lane = lane_id();
  const uint64_t below_me = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  int used = 0;
  for (int t0 = k0; t0 < k1; t0 += kTile32) {
    const int mm = min(kTile32, k1 - t0);
    float4 c[kQ];
    bool keep[kQ];
    uint64_t bal[kQ];
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
      const int j = q * kBS + threadIdx.x;
      keep[q] = false;
      if (j < mm) {
        c[q] = coef[t0 + j];
        keep[q] = term_max(c[q], xlo, xhi) >= thr;
      }
      bal[q] = __ballot(keep[q]);
    }
    __syncthreads();  // previous tile consumed, cnt free
    if (lane == 0)
#pragma unroll
      for (int q = 0; q < kQ; ++q) cnt[q * kW + wid] = __popcll(bal[q]);
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
      int mine = 0;
#pragma unroll
      for (int w = 0; w < kW; ++w) {
        const int n = cnt[q * kW + w];
        if (w < wid) mine += n;
        tot += n;
      }
      if (keep[q]) tile[pre + mine + __popcll(bal[q] & below_me)] = c[q];
      pre = tot;
    }
    __syncthreads();
    lse32_tile(L, tile, tot);
    used += tot;
  }
  return used;
}

template <int R>
__device__ __forceinline__ void lse32_end(const Lse32<R>& L, const tpe_seg& S, float (&out)[R]) {
  const float C = (float)S.cmax;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const float l2 = __builtin_amdgcn_logf(L.s[r]);  // log2
    out[r] = (L.fast ? (l2 + C) : (L.m[r] + l2 + C)) * kLn2f;
  }
}

template <int R>
__device__ __forceinline__ void lse32(const float4* __restrict__ coef, const tpe_seg& S,
                                      const float (&y)[R], float (&out)[R], float4* tile) {
  Lse32<R> L;
  lse32_begin(L, coef, S, y);
  lse32_accum(L, coef, 0, S.n_obs + 1, tile);
  lse32_end(L, S, out);
}

// exact online log-sum-exp, fp64 (parity mode)
template <int R>
__device__ __forceinline__ void lse64(const double4* __restrict__ coef, const tpe_seg& S,
                                      const double (&y)[R], double (&out)[R], double4* tile) {
  const int nc = S.n_obs + 1;
  double s[R], m[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    s[r] = 0.0;
    m[r] = -INFINITY;
  }
  for (int t0 = 0; t0 < nc; t0 += kTile64) {
    const int mm = min(kTile64, nc - t0);
    __syncthreads();
    for (int j = threadIdx.x; j < mm; j += kBS) tile[j] = coef[t0 + j];
    __syncthreads();
    for (int k = 0; k < mm; ++k) {
      const double4 c = tile[k];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const double t = (y[r] - c.x) * c.y;
        const double v = -0.5 * (t * t) + c.z;
        // one exp per pair on every lane: a branch per lane would run the
        // (software) fp64 exp twice whenever the wave diverges.  Same values
        // as s*exp(m-v)+1 (new max) / s+exp(v-m), NaN included.
        const bool up = v > m[r];
        const double e = exp(up ? m[r] - v : v - m[r]);
        s[r] = up ? s[r] * e + 1.0 : s[r] + e;
        m[r] = up ? v : m[r];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) out[r] = log(s[r]) + m[r];
}

// ---------------------------------------------------------------------------
// continuous, unquantized: sample/read + score + argmax
// ---------------------------------------------------------------------------
template <bool INJ>
__global__ __launch_bounds__(kBS) void k_score32(
    const tpe_job* __restrict__ jobs, const tpe_seg* __restrict__ segs,
    const double* __restrict__ mu, const double* __restrict__ sigma,
    const double* __restrict__ wcdf, const float4* __restrict__ coef32,
    const double* __restrict__ cand, double* __restrict__ out_bl, double* __restrict__ out_al,
    double* __restrict__ out_x, tpe_best* __restrict__ partial) {
  __shared__ float4 tile[kTile32];
  __shared__ MixLds s_mix;
  __shared__ BestT red[kBS / kWave];
  const tpe_job J = jobs[blockIdx.y];
  tpe_best* P = partial + (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  const int64_t base = (int64_t)blockIdx.x * (kBS * kR32);
  if (base >= J.n_cand) {
    if (threadIdx.x == 0) *P = empty_best();
    return;
  }
  const tpe_seg SB = segs[J.below], SA = segs[J.above];
  const bool lgmm = J.family == TPE_LGMM1;
  const bool lo_on = J.flags & TPE_F_LOW, hi_on = J.flags & TPE_F_HIGH;
  // x: the given value (INJ) or the fp32 draw in the mixture's coordinate
  // (log x for LGMM1, whose value is exp(y) evaluated in fp64: log(value) is
  // then y itself, see cand_value in tpe_table.hip)
  float x[kR32], y[kR32];
  if (INJ) {
#pragma unroll
    for (int r = 0; r < kR32; ++r) {
      const int64_t li = base + r * kBS + threadIdx.x;
      x[r] = li < J.n_cand ? (float)cand[J.cand_off + li] : 1.0f;
    }
  } else {
    const Mix M = stage_mix(SB, wcdf, mu, sigma, s_mix);
#pragma unroll
    for (int r = 0; r < kR32; ++r) {
      const int64_t li = base + r * kBS + threadIdx.x;
      x[r] = li < J.n_cand ? draw32(M, J.key, J.cand_base + li, lo_on, hi_on, bound32(J.low),
                                    bound32(J.high))
                           : 1.0f;
    }
  }
#pragma unroll
  for (int r = 0; r < kR32; ++r) {
    const int64_t li = base + r * kBS + threadIdx.x;
    if (li < J.n_cand)
      y[r] = (lgmm && INJ) ? __logf(x[r]) : x[r];
    else
      y[r] = (float)SA.center;  // inactive lanes sit on the prior mean
  }
  float lb[kR32], la[kR32];
  lse32<kR32>(coef32 + SB.comp_off, SB, y, lb, tile);
  lse32<kR32>(coef32 + SA.comp_off, SA, y, la, tile);
  BestT b{0.0, -1, 0.0};
#pragma unroll
  for (int r = 0; r < kR32; ++r) {
    const int64_t li = base + r * kBS + threadIdx.x;
    if (li >= J.n_cand) continue;
    double bl = lb[r], al = la[r];
    if (lgmm) {  // lognormal_lpdf's -log(x) (tpe.py:214-216)
      bl -= (double)y[r];
      al -= (double)y[r];
    }
    const double v = (lgmm && !INJ) ? exp((double)x[r]) : (double)x[r];
    const int64_t o = J.out_off + li;
    if (out_bl) out_bl[o] = bl;
    if (out_al) out_al[o] = al;
    if (out_x) out_x[o] = v;
    best_update(b, bl - al, J.cand_base + li, v);
  }
  b = block_best<kBS>(b, red);
  if (threadIdx.x == 0) *P = tpe_best{b.score, b.index, b.value, 0};
}

template <bool INJ>
__global__ __launch_bounds__(kBS) void k_score64(
    const tpe_job* __restrict__ jobs, const tpe_seg* __restrict__ segs,
    const double* __restrict__ mu, const double* __restrict__ sigma,
    const double* __restrict__ wcdf, const double4* __restrict__ coef64,
    const double* __restrict__ cand, double* __restrict__ out_bl, double* __restrict__ out_al,
    double* __restrict__ out_x, tpe_best* __restrict__ partial) {
  __shared__ double4 tile[kTile64];
  __shared__ MixLds s_mix;
  __shared__ BestT red[kBS / kWave];
  const tpe_job J = jobs[blockIdx.y];
  tpe_best* P = partial + (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  const int64_t base = (int64_t)blockIdx.x * (kBS * kR64);
  if (base >= J.n_cand) {
    if (threadIdx.x == 0) *P = empty_best();
    return;
  }
  const tpe_seg SB = segs[J.below], SA = segs[J.above];
  const bool lgmm = J.family == TPE_LGMM1;
  const bool lo_on = J.flags & TPE_F_LOW, hi_on = J.flags & TPE_F_HIGH;
  double x[kR64], y[kR64];
  if (INJ) {
#pragma unroll
    for (int r = 0; r < kR64; ++r) {
      const int64_t li = base + r * kBS + threadIdx.x;
      x[r] = li < J.n_cand ? cand[J.cand_off + li] : 1.0;
    }
  } else {
    const Mix M = stage_mix(SB, wcdf, mu, sigma, s_mix);
#pragma unroll
    for (int r = 0; r < kR64; ++r) {
      const int64_t li = base + r * kBS + threadIdx.x;
      double v = 1.0;
      if (li < J.n_cand) {
        v = draw64(M, J.key, J.cand_base + li, lo_on, hi_on, J.low, J.high);
        if (lgmm) v = exp(v);
      }
      x[r] = v;
    }
  }
#pragma unroll
  for (int r = 0; r < kR64; ++r) {
    const int64_t li = base + r * kBS + threadIdx.x;
    y[r] = li < J.n_cand ? (lgmm ? log(x[r]) : x[r]) : SA.prior_mu;
  }
  double lb[kR64], la[kR64];
  lse64<kR64>(coef64 + SB.comp_off, SB, y, lb, tile);
  lse64<kR64>(coef64 + SA.comp_off, SA, y, la, tile);
  BestT b{0.0, -1, 0.0};
#pragma unroll
  for (int r = 0; r < kR64; ++r) {
    const int64_t li = base + r * kBS + threadIdx.x;
    if (li >= J.n_cand) continue;
    double bl = lb[r], al = la[r];
    if (lgmm) {
      bl -= y[r];
      al -= y[r];
    }
    const int64_t o = J.out_off + li;
    if (out_bl) out_bl[o] = bl;
    if (out_al) out_al[o] = al;
    if (out_x) out_x[o] = x[r];
    best_update(b, bl - al, J.cand_base + li, x[r]);
  }
  b = block_best<kBS>(b, red);
  if (threadIdx.x == 0) *P = tpe_best{b.score, b.index, b.value, 0};
}

// ---------------------------------------------------------------------------
// continuous, unquantized, sorted + pruned (fp32)
// ---------------------------------------------------------------------------
constexpr int kNB = 512;                 // value bins per label
constexpr int kSortR = 16;               // candidates per thread in count / scatter
constexpr int kSortPer = kBS * kSortR;   // candidates per count / scatter block (4096)

__device__ __forceinline__ int bin_of(float y, float lo, float scale) {
  float t = (y - lo) * scale;
  t = fminf(fmaxf(t, 0.0f), (float)(kNB - 1));  // NaN -> 0
  return (int)t;
}

// the candidate exactly as k_score32<false> draws it, in the mixture's
// coordinate (log x for LGMM1: its value is exp(y) in fp64)
__device__ __forceinline__ float cand32(const Mix& M, const tpe_job& J, int64_t li, bool lo_on,
                                        bool hi_on) {
  return draw32(M, J.key, J.cand_base + li, lo_on, hi_on, bound32(J.low), bound32(J.high));
}

// K1: draw every candidate once (kept in `gen`, generation order, coalesced)
// and count them per (block, value bin)
__global__ __launch_bounds__(kBS) void k_sort_count(
    const tpe_job* __restrict__ jobs, const tpe_seg* __restrict__ segs,
    const double* __restrict__ mu, const double* __restrict__ sigma,
    const double* __restrict__ wcdf, uint32_t* __restrict__ counts, float* __restrict__ gen) {
  __shared__ uint32_t h[kNB];
  __shared__ MixLds s_mix;
  const tpe_job J = jobs[blockIdx.y];
  const int64_t base = (int64_t)blockIdx.x * kSortPer;
  if (base >= J.n_cand) return;
  for (int i = threadIdx.x; i < kNB; i += kBS) h[i] = 0u;
  const Mix M = stage_mix(segs[J.below], wcdf, mu, sigma, s_mix);
  __syncthreads();
  const bool lo_on = J.flags & TPE_F_LOW, hi_on = J.flags & TPE_F_HIGH;
  const float lo = (float)J.bin_lo, scale = (float)(kNB / (J.bin_hi - J.bin_lo));
  for (int r = 0; r < kSortR; ++r) {
    const int64_t li = base + r * kBS + threadIdx.x;
    if (li >= J.n_cand) break;
    const float y = cand32(M, J, li, lo_on, hi_on);
    gen[J.sort_off + li] = y;
    atomicAdd(&h[bin_of(y, lo, scale)], 1u);
  }
  __syncthreads();
  uint32_t* row = counts + 2 * J.cnt_off + (int64_t)blockIdx.x * kNB;
  for (int i = threadIdx.x; i < kNB; i += kBS) row[i] = h[i];
}

// K2: exclusive offsets of every (block, bin) run in bin-major order.  The
// count matrix is cut into chunks of kScanChunk blocks: column sums per chunk
// (K2a), one scan over (bin, chunk) per job (K2b), offsets per chunk (K2c).
constexpr int kScanChunk = 32;

__device__ __forceinline__ int64_t sort_nblk(const tpe_job& J) {
  return (J.n_cand + kSortPer - 1) / kSortPer;
}

__global__ __launch_bounds__(kNB) void k_sort_colsum(const tpe_job* __restrict__ jobs,
                                                     uint32_t* __restrict__ counts) {
  const tpe_job J = jobs[blockIdx.y];
  const int64_t nblk = sort_nblk(J);
  const int64_t b0 = (int64_t)blockIdx.x * kScanChunk;
  if (b0 >= nblk) return;
  const int64_t b1 = min(nblk, b0 + kScanChunk);
  const uint32_t* C = counts + 2 * J.cnt_off;
  uint32_t* S = counts + 2 * J.cnt_off + 2 * nblk * kNB;
  uint32_t t = 0;
#pragma unroll 8
  for (int64_t b = b0; b < b1; ++b) t += C[b * kNB + threadIdx.x];
  S[blockIdx.x * kNB + threadIdx.x] = t;
}

__global__ __launch_bounds__(kNB) void k_sort_scan(const tpe_job* __restrict__ jobs,
                                                   uint32_t* __restrict__ counts) {
  __shared__ uint32_t tot[kNB];
  const tpe_job J = jobs[blockIdx.x];
  const int64_t nblk = sort_nblk(J);
  const int nch = (int)((nblk + kScanChunk - 1) / kScanChunk);
  uint32_t* S = counts + 2 * J.cnt_off + 2 * nblk * kNB;
  const int bin = threadIdx.x;
  uint32_t t = 0;
  for (int c = 0; c < nch; ++c) t += S[c * kNB + bin];
  tot[bin] = t;
  __syncthreads();
  // inclusive Hillis-Steele scan over bins
  for (int d = 1; d < kNB; d <<= 1) {
    const uint32_t v = bin >= d ? tot[bin - d] : 0u;
    __syncthreads();
    tot[bin] += v;
    __syncthreads();
  }
  uint32_t run = tot[bin] - t;  // exclusive
  for (int c = 0; c < nch; ++c) {
    const uint32_t v = S[c * kNB + bin];
    S[c * kNB + bin] = run;
    run += v;
  }
}

__global__ __launch_bounds__(kNB) void k_sort_offsets(const tpe_job* __restrict__ jobs,
                                                      uint32_t* __restrict__ counts) {
  const tpe_job J = jobs[blockIdx.y];
  const int64_t nblk = sort_nblk(J);
  const int64_t b0 = (int64_t)blockIdx.x * kScanChunk;
  if (b0 >= nblk) return;
  const int64_t b1 = min(nblk, b0 + kScanChunk);
  const uint32_t* C = counts + 2 * J.cnt_off;
  uint32_t* O = counts + 2 * J.cnt_off + nblk * kNB;
  const uint32_t* S = counts + 2 * J.cnt_off + 2 * nblk * kNB;
  uint32_t run = S[blockIdx.x * kNB + threadIdx.x];
  for (int64_t b = b0; b < b1; ++b) {
    O[b * kNB + threadIdx.x] = run;
    run += C[b * kNB + threadIdx.x];
  }
}

// K3: bucket the block's candidates in LDS by bin, then write each bin's run
// contiguously to its global slot range (coalesced runs instead of scattered
// 4-byte stores)
__global__ __launch_bounds__(kBS) void k_sort_scatter(const tpe_job* __restrict__ jobs,
                                                      const uint32_t* __restrict__ counts,
                                                      const float* __restrict__ gen,
                                                      float* __restrict__ sorted_x,
                                                      uint32_t* __restrict__ sorted_i) {
  __shared__ uint32_t lstart[kNB], cur[kNB], goff[kNB];
  __shared__ float sx[kSortPer];
  __shared__ uint32_t si[kSortPer];
  __shared__ uint16_t sb[kSortPer];
  __shared__ uint32_t part[kBS];
  const tpe_job J = jobs[blockIdx.y];
  const int64_t base = (int64_t)blockIdx.x * kSortPer;
  if (base >= J.n_cand) return;
  const int64_t nblk = (J.n_cand + kSortPer - 1) / kSortPer;
  const uint32_t* C = counts + 2 * J.cnt_off + (int64_t)blockIdx.x * kNB;
  const uint32_t* O = counts + 2 * J.cnt_off + nblk * kNB + (int64_t)blockIdx.x * kNB;
  // local exclusive scan of this block's bin counts (kNB = 2 * kBS)
  const uint32_t c0 = C[2 * threadIdx.x], c1 = C[2 * threadIdx.x + 1];
  part[threadIdx.x] = c0 + c1;
  goff[2 * threadIdx.x] = O[2 * threadIdx.x];
  goff[2 * threadIdx.x + 1] = O[2 * threadIdx.x + 1];
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t acc = 0;
    for (int t = 0; t < kBS; ++t) {
      const uint32_t c = part[t];
      part[t] = acc;
      acc += c;
    }
  }
  __syncthreads();
  lstart[2 * threadIdx.x] = cur[2 * threadIdx.x] = part[threadIdx.x];
  lstart[2 * threadIdx.x + 1] = cur[2 * threadIdx.x + 1] = part[threadIdx.x] + c0;
  __syncthreads();
  const float lo = (float)J.bin_lo, scale = (float)(kNB / (J.bin_hi - J.bin_lo));
  const int n = (int)min((int64_t)kSortPer, J.n_cand - base);
  for (int r = 0; r < kSortR; ++r) {
    const int e = r * kBS + threadIdx.x;
    if (e >= n) break;
    const float x = gen[J.sort_off + base + e];  // (the mixture coordinate)
    const int b = bin_of(x, lo, scale);
    const uint32_t lp = atomicAdd(&cur[b], 1u);
    sx[lp] = x;
    si[lp] = (uint32_t)(base + e);
    sb[lp] = (uint16_t)b;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < n; e += kBS) {
    const int b = sb[e];
    const uint32_t g = goff[b] + (uint32_t)(e - lstart[b]);
    sorted_x[J.sort_off + g] = sx[e];
    sorted_i[J.sort_off + g] = si[e];
  }
}

// first k with a[k] > v (a non-decreasing)
__device__ __forceinline__ int first_greater(const float* a, int n, float v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] > v) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(kBS) void k_score_sorted(
    const tpe_job* __restrict__ jobs, const tpe_seg* __restrict__ segs,
    const float4* __restrict__ coef32, const float4* __restrict__ coef32n,
    const float4* __restrict__ wide32, const float* __restrict__ pm,
    const float* __restrict__ sm, const float* __restrict__ sorted_x,
    const uint32_t* __restrict__ sorted_i, tpe_best* __restrict__ partial,
    unsigned long long* __restrict__ pairs) {
  __shared__ float4 tile[kTile32];
  __shared__ BestT red[kBS / kWave];
  __shared__ float fred[3][kBS / kWave];
  __shared__ int win[2];
  __shared__ float yr[2];
  __shared__ int cnt[kTile32 / kWave];
  __shared__ float lred[2][kBS / kWave];
  const tpe_job J = jobs[blockIdx.y];
  tpe_best* P = partial + (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  const int64_t base = (int64_t)blockIdx.x * (kBS * kR32);
  if (base >= J.n_cand) {
    if (threadIdx.x == 0) *P = empty_best();
    return;
  }
  const tpe_seg SB = segs[J.below], SA = segs[J.above];
  const bool lgmm = J.family == TPE_LGMM1;
  float x[kR32], y[kR32];
  uint32_t li[kR32];
  float ymin = INFINITY, ymax = -INFINITY, vmin = INFINITY;
  const float4 cp = coef32[SA.comp_off + SA.prior_pos];
  const float cen = (float)SA.center;
  int nvalid = 0;
#pragma unroll
  for (int r = 0; r < kR32; ++r) {
    const int64_t p = base + r * kBS + threadIdx.x;
    if (p < J.n_cand) {
      x[r] = sorted_x[J.sort_off + p];  // the mixture coordinate
      li[r] = sorted_i[J.sort_off + p];
      y[r] = x[r];
      ymin = fminf(ymin, y[r]);
      ymax = fmaxf(ymax, y[r]);
      const float t = fmaf(y[r] - cen, cp.x, cp.y);
      vmin = fminf(vmin, fmaf(-t, t, cp.z));
      ++nvalid;
    } else {
      x[r] = 1.0f;
      li[r] = 0;
      y[r] = cen;
    }
  }
  // block reductions: y range and the smallest prior term
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    ymin = fminf(ymin, __shfl_xor(ymin, off, kWave));
    ymax = fmaxf(ymax, __shfl_xor(ymax, off, kWave));
    vmin = fminf(vmin, __shfl_xor(vmin, off, kWave));
  }
  const int wid = threadIdx.x / kWave;
  if (lane_id() == 0) {
    fred[0][wid] = ymin;
    fred[1][wid] = ymax;
    fred[2][wid] = vmin;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = fred[0][0], b = fred[1][0], c = fred[2][0];
    for (int k = 1; k < kBS / kWave; ++k) {
      a = fminf(a, fred[0][k]);
      b = fmaxf(b, fred[1][k]);
      c = fminf(c, fred[2][k]);
    }
    const int nc = SA.n_obs + 1;
    yr[0] = a;
    yr[1] = b;
    if (c >= (float)SA.lglob) {
      const float* PM = pm + SA.comp_off;
      const float* SMn = sm + SA.comp_off;
      win[0] = first_greater(PM, nc, a);           // first k with mu+r > ymin
      win[1] = first_greater(SMn, nc, b) - 1;      // last k with mu-r < ymax... (sm < b)
    } else {
      win[0] = -1;  // far-out block: every component, unmasked
      win[1] = nc - 1;
    }
  }
  __syncthreads();
  const int k_lo = win[0], k_hi = win[1];

  float lb[kR32], la[kR32];
  lse32<kR32>(coef32 + SB.comp_off, SB, y, lb, tile);
  Lse32<kR32> L;
  lse32_begin(L, coef32 + SA.comp_off, SA, y);
  int64_t evaluated;
  if (k_lo < 0) {
    lse32_accum(L, coef32 + SA.comp_off, 0, SA.n_obs + 1, tile);
    evaluated = SA.n_obs + 1;
  } else {
    // Block threshold.  Every candidate of the block has log2(sum) >= Lb =
    // log2(sum_k 2^min_block(v_k)) over the window + wide components.  A
    // component whose largest term over the block is below Lb - margin adds
    // less than 2^-margin of the sum; with margin = log2(n) + 20 all dropped
    // components together change the sum by < 2^-20 (relative).  Components
    // outside the window were already below 2^(lglob - 40) (tpe_fit.hip).
    const float xlo = yr[0] - cen, xhi = yr[1] - cen;
    float m = -INFINITY, sacc = 0.0f;
    auto add = [&](const float4 cc) {
      const float v = term_min(cc, xlo, xhi);
      if (v > m) {
        sacc = sacc * __builtin_amdgcn_exp2f(m - v) + 1.0f;
        m = v;
      } else if (v > -INFINITY) {
        sacc += __builtin_amdgcn_exp2f(v - m);
      }
    };
    for (int k = k_lo + (int)threadIdx.x; k <= k_hi; k += kBS) add(coef32n[SA.comp_off + k]);
    for (int k = threadIdx.x; k < SA.n_wide; k += kBS) add(wide32[SA.comp_off + k]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float mo = __shfl_xor(m, off, kWave), so = __shfl_xor(sacc, off, kWave);
      const float mn = fmaxf(m, mo);
      sacc = (mn == -INFINITY) ? 0.0f
                               : sacc * __builtin_amdgcn_exp2f(m - mn) + so * __builtin_amdgcn_exp2f(mo - mn);
      m = mn;
    }
    if (lane_id() == 0) {
      lred[0][wid] = m;
      lred[1][wid] = sacc;
    }
    __syncthreads();
    float mb = -INFINITY;
    for (int w = 0; w < kBS / kWave; ++w) mb = fmaxf(mb, lred[0][w]);
    float sb = 0.0f;
    for (int w = 0; w < kBS / kWave; ++w)
      if (lred[0][w] > -INFINITY) sb += lred[1][w] * __builtin_amdgcn_exp2f(lred[0][w] - mb);
    const float margin = __builtin_amdgcn_logf((float)(SA.n_obs + 1)) + 20.0f;
    const float thr = (mb > -INFINITY) ? mb + __builtin_amdgcn_logf(sb) - margin : -INFINITY;
    evaluated = 0;
    if (k_hi >= k_lo)
      evaluated = lse32_accum_pruned(L, coef32n + SA.comp_off, k_lo, k_hi + 1, tile, cnt, xlo,
                                     xhi, thr);
    lse32_accum(L, wide32 + SA.comp_off, 0, SA.n_wide, tile);
    evaluated += SA.n_wide;
  }
  lse32_end(L, SA, la);

  BestT b{0.0, -1, 0.0};
#pragma unroll
  for (int r = 0; r < kR32; ++r) {
    const int64_t p = base + r * kBS + threadIdx.x;
    if (p >= J.n_cand) continue;
    double bl = lb[r], al = la[r];
    if (lgmm) {  // lognormal_lpdf's -log(x) (tpe.py:214-216): log of exp(y) is y
      bl -= (double)y[r];
      al -= (double)y[r];
    }
    best_update(b, bl - al, J.cand_base + (int64_t)li[r],
                lgmm ? exp((double)x[r]) : (double)x[r]);
  }
  b = block_best<kBS>(b, red);
  if (threadIdx.x == 0) {
    *P = tpe_best{b.score, b.index, b.value, 0};
    if (pairs) {
      const int64_t n = min((int64_t)(kBS * kR32), J.n_cand - base);
      atomicAdd(pairs, (unsigned long long)(n * (evaluated + SB.n_obs + 1)));
    }
  }
  (void)nvalid;
}

// ---------------------------------------------------------------------------
// sampler only
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBS) void k_sample(const tpe_job* __restrict__ jobs,
                                                const tpe_seg* __restrict__ segs,
                                                const double* __restrict__ mu,
                                                const double* __restrict__ sigma,
                                                const double* __restrict__ wcdf,
                                                double* __restrict__ out_x) {
  __shared__ MixLds s_mix;
  __shared__ float s_stage[kLatR * kBS];
  __shared__ uint16_t s_list[(kBS / kWave) * kRetryList];
  const tpe_job J = jobs[blockIdx.y];
  const int64_t base = (int64_t)blockIdx.x * (kBS * kLatR);
  if (base >= J.n_cand) return;
  const Mix M = stage_mix(segs[J.below], wcdf, mu, sigma, s_mix);
  const bool lgmm = J.family == TPE_LGMM1;
  const bool lo_on = J.flags & TPE_F_LOW, hi_on = J.flags & TPE_F_HIGH;
  if (sizeof(T) == 4) {
    // the fp32 stream exactly as the scorers draw it: kLatR consecutive
    // candidates per thread through draw32_pairs (the table scorer's and the
    // DRAW32 lattice sampler's code); LGMM1 values as exp(y) in fp64 for
    // unquantized labels (the scorers' values), __expf(y) for quantized ones
    // (the lattice sampler's slots)
    const bool quant = J.flags & TPE_F_QUANT;
    const int64_t t0 = base + (int64_t)threadIdx.x * kLatR;
    const int nv = (int)max((int64_t)0, min((int64_t)kLatR, J.n_cand - t0));
    float x[kLatR];
    draw32_pairs<kLatR>(M, J.key, J.cand_base + t0, nv, lo_on, hi_on, bound32(J.low),
                        bound32(J.high), lgmm && quant,
                        s_stage + (threadIdx.x / kWave) * (kLatR * kWave),
                        s_list + (threadIdx.x / kWave) * kRetryList, x);
#pragma unroll
    for (int r = 0; r < kLatR; ++r) {
      if (r >= nv) continue;
      double v = (lgmm && !quant) ? exp((double)x[r]) : (double)x[r];
      if (quant) v = rint(v / J.q) * J.q;
      out_x[J.out_off + t0 + r] = v;
    }
    return;
  }
  for (int r = 0; r < kLatR; ++r) {
    const int64_t li = base + r * kBS + threadIdx.x;
    if (li >= J.n_cand) break;
    double v = draw64(M, J.key, J.cand_base + li, lo_on, hi_on, J.low, J.high);
    if (lgmm) v = exp(v);
    if (J.flags & TPE_F_QUANT) v = rint(v / J.q) * J.q;
    out_x[J.out_off + li] = v;
  }
}

__global__ void k_combine(const tpe_best* __restrict__ sets, int n_sets, int n_labels,
                          tpe_best* __restrict__ out) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= n_labels) return;
  tpe_best b = sets[l];
  int64_t n = b.n_scored;
  bool inexact = n < 0;  // a set whose exact decision is still owed (band overflow)
  for (int s = 1; s < n_sets; ++s) {
    const tpe_best o = sets[(int64_t)s * n_labels + l];
    n += o.n_scored;
    inexact = inexact || o.n_scored < 0;
    if (better(o.score, o.index, b.score, b.index)) b = o;
  }
  b.n_scored = inexact ? -1 : n;  // -1 travels: every rank sees the label is owed
  out[l] = b;
}

}  // namespace
}  // namespace tpe

using namespace tpe;

extern "C" int64_t tpe_score_partials(const tpe_job* host_jobs, int n_jobs) {
  // the larger of the fp32 and fp64 grids
  return (int64_t)n_jobs * tiles_per_job(host_jobs, n_jobs, kBS * kR64);
}

extern "C" int tpe_score_continuous(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                                    const tpe_seg* segs, const double* w, const double* mu,
                                    const double* sigma, const double* wcdf,
                                    const double* coef64, const float* coef32,
                                    const double* cand, int precision, double* out_bl,
                                    double* out_al, double* out_x, tpe_best* partial,
                                    int64_t n_partial, tpe_best* best, void* stream) {
  (void)w;
  if (!check_jobs("tpe_score_continuous", host_jobs, n_jobs)) return TPE_E_ARG;
  if (n_jobs == 0) return TPE_OK;
  if (precision != 32 && precision != 64) {
    set_error("tpe_score_continuous: precision must be 32 or 64, got %d", precision);
    return TPE_E_ARG;
  }
  bool inj = false;
  if (!check_gmm_jobs("tpe_score_continuous", host_jobs, n_jobs, 65535, 0, &inj)) return TPE_E_ARG;
  if (!jobs || !segs || !mu || !sigma || !wcdf || !partial || !best || (inj && !cand) ||
      (precision == 32 ? !coef32 : !coef64)) {
    set_error("tpe_score_continuous: null pointer");
    return TPE_E_ARG;
  }
  const int R = precision == 32 ? kR32 : kR64;
  const int64_t gx = tiles_per_job(host_jobs, n_jobs, (int64_t)kBS * R);
  if (!check_partials("tpe_score_continuous", n_partial, gx * n_jobs)) return TPE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)gx, (unsigned)n_jobs);
  dispatch_bool(inj, [&](auto INJ) {
    if (precision == 32)
      hipLaunchKernelGGL(k_score32<decltype(INJ)::value>, grid, dim3(kBS), 0, st, jobs, segs, mu,
                         sigma, wcdf, reinterpret_cast<const float4*>(coef32), cand, out_bl,
                         out_al, out_x, partial);
    else
      hipLaunchKernelGGL(k_score64<decltype(INJ)::value>, grid, dim3(kBS), 0, st, jobs, segs, mu,
                         sigma, wcdf, reinterpret_cast<const double4*>(coef64), cand, out_bl,
                         out_al, out_x, partial);
  });
  launch_reduce(jobs, partial, gx, best, n_jobs, st);
  return check_launch("tpe_score_continuous");
}

extern "C" int tpe_sample(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                          const tpe_seg* segs, const double* mu, const double* sigma,
                          const double* wcdf, int precision, double* out_x, void* stream) {
  if (!check_jobs("tpe_sample", host_jobs, n_jobs)) return TPE_E_ARG;
  if (n_jobs == 0) return TPE_OK;
  if (!jobs || !segs || !mu || !sigma || !wcdf || !out_x || (precision != 32 && precision != 64)) {
    set_error("tpe_sample: bad arguments");
    return TPE_E_ARG;
  }
  for (int i = 0; i < n_jobs; ++i)
    if (host_jobs[i].family == TPE_CAT) {
      set_error("tpe_sample: categorical jobs are sampled by tpe_score_categorical");
      return TPE_E_ARG;
    }
  const int64_t gx = tiles_per_job(host_jobs, n_jobs, (int64_t)kBS * kLatR);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)gx, (unsigned)n_jobs);
  if (precision == 32)
    hipLaunchKernelGGL(k_sample<float>, grid, dim3(kBS), 0, st, jobs, segs, mu, sigma, wcdf, out_x);
  else
    hipLaunchKernelGGL(k_sample<double>, grid, dim3(kBS), 0, st, jobs, segs, mu, sigma, wcdf,
                       out_x);
  return check_launch("tpe_sample");
}

extern "C" int tpe_best_combine(const tpe_best* sets, int n_sets, int n_labels, tpe_best* out,
                                void* stream) {
  if (n_sets <= 0 || n_labels < 0 || (n_labels > 0 && (!sets || !out))) {
    set_error("tpe_best_combine: bad arguments");
    return TPE_E_ARG;
  }
  if (n_labels == 0) return TPE_OK;
  hipLaunchKernelGGL(k_combine, dim3((n_labels + kBS - 1) / kBS), dim3(kBS), 0,
                     (hipStream_t)stream, sets, n_sets, n_labels, out);
  return check_launch("tpe_best_combine");
}

extern "C" int64_t tpe_sort_layout(int64_t n_cand, int64_t* sorted_slots) {
  // u32 words used = 2 x the returned value: the count matrix (blocks x
  // bins), the run offsets (same shape), then per-chunk column sums
  if (sorted_slots) *sorted_slots = n_cand;
  const int64_t nblk = (n_cand + kSortPer - 1) / kSortPer;
  const int64_t nch = (nblk + kScanChunk - 1) / kScanChunk;
  return nblk * (int64_t)kNB + (nch * (int64_t)kNB + 1) / 2;
}

static bool check_sorted_jobs(const char* fn, const tpe_job* host_jobs, int n_jobs) {
  if (!check_jobs(fn, host_jobs, n_jobs)) return false;
  for (int i = 0; i < n_jobs; ++i) {
    const tpe_job& j = host_jobs[i];
    if (!check_gmm_job(fn, i, j, kJobSampled)) return false;
    if (!(j.bin_hi > j.bin_lo) || j.n_cand > 0xFFFFFFFFll) {
      set_error("%s: job %d has an empty bin range or > 2^32 candidates", fn, i);
      return false;
    }
  }
  return true;
}

extern "C" int tpe_sort_candidates(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                                   const tpe_seg* segs, const double* mu, const double* sigma,
                                   const double* wcdf, uint32_t* counts, float* gen,
                                   float* sorted_x, uint32_t* sorted_i, void* stream) {
  if (!check_sorted_jobs("tpe_sort_candidates", host_jobs, n_jobs)) return TPE_E_ARG;
  if (n_jobs == 0) return TPE_OK;
  if (!jobs || !segs || !mu || !sigma || !wcdf || !counts || !gen || !sorted_x || !sorted_i) {
    set_error("tpe_sort_candidates: null pointer");
    return TPE_E_ARG;
  }
  const int64_t gs = tiles_per_job(host_jobs, n_jobs, (int64_t)kSortPer);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_sort_count, dim3((unsigned)gs, (unsigned)n_jobs), dim3(kBS), 0, st, jobs,
                     segs, mu, sigma, wcdf, counts, gen);
  const int64_t gch = (gs + kScanChunk - 1) / kScanChunk;
  hipLaunchKernelGGL(k_sort_colsum, dim3((unsigned)gch, (unsigned)n_jobs), dim3(kNB), 0, st, jobs,
                     counts);
  hipLaunchKernelGGL(k_sort_scan, dim3(n_jobs), dim3(kNB), 0, st, jobs, counts);
  hipLaunchKernelGGL(k_sort_offsets, dim3((unsigned)gch, (unsigned)n_jobs), dim3(kNB), 0, st, jobs,
                     counts);
  hipLaunchKernelGGL(k_sort_scatter, dim3((unsigned)gs, (unsigned)n_jobs), dim3(kBS), 0, st, jobs,
                     counts, gen, sorted_x, sorted_i);
  return check_launch("tpe_sort_candidates");
}

extern "C" int tpe_score_sorted(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                                const tpe_seg* segs, const float* coef32, const float* coef32n,
                                const float* wide32, const float* pm, const float* sm,
                                const float* sorted_x, const uint32_t* sorted_i,
                                tpe_best* partial, int64_t n_partial, tpe_best* best,
                                uint64_t* pairs, void* stream) {
  if (!check_sorted_jobs("tpe_score_sorted", host_jobs, n_jobs)) return TPE_E_ARG;
  if (n_jobs == 0) return TPE_OK;
  if (!jobs || !segs || !coef32 || !coef32n || !wide32 || !pm || !sm || !sorted_x ||
      !sorted_i || !partial || !best) {
    set_error("tpe_score_sorted: null pointer");
    return TPE_E_ARG;
  }
  const int64_t gx = tiles_per_job(host_jobs, n_jobs, (int64_t)kBS * kR32);
  if (gx * n_jobs > n_partial) {
    set_error("tpe_score_sorted: partial workspace too small");
    return TPE_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_score_sorted, dim3((unsigned)gx, (unsigned)n_jobs), dim3(kBS), 0, st, jobs,
                     segs, reinterpret_cast<const float4*>(coef32),
                     reinterpret_cast<const float4*>(coef32n),
                     reinterpret_cast<const float4*>(wide32), pm, sm, sorted_x, sorted_i, partial,
                     (unsigned long long*)pairs);
  launch_reduce(jobs, partial, gx, best, n_jobs, st);
  return check_launch("tpe_score_sorted");
}
