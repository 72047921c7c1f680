// tpe_pruned64.hip -- exact fp64 scoring with component pruning (the parity
// mode at large M): GMM1_lpdf / LGMM1_lpdf (hyperopt/tpe.py:117-180, 265-307)
// and broadcast_best's argmax (tpe.py:649-658) over the components the
// table's plan (tpe_table.hip) cannot rule out.
//
// Exports: tpe_pruned64_partials, tpe_score_pruned64, tpe_exp_neg64_check
// (the sum's exp on a caller's arguments, for the tests).
#include "tpe_table.hpp"

namespace tpe {
namespace {
constexpr double kDrawZ64 = 8.7;     // |z| of an fp64 Box-Muller draw (53-bit uniforms) is < 8.6
constexpr double kTauExact = 40.0;   // margin of the pruned exact fp64 scorer: e^-40 < 5e-18

// ---------------------------------------------------------------------------
// exact fp64 scoring with component pruning (the parity mode at large M)
// ---------------------------------------------------------------------------
// The plan (k_table_plan1/2 with margin kTauExact) gives every mixture a
// floor T: a component whose term stays below T over the whole candidate
// range can add at most e^-40 of the prior component's term, itself a lower
// bound of the sum (exactly the table's exclusion rule with a wider margin),
// and reach windows over the sorted means.  A candidate sums, in fp64 with
// the online log-sum-exp of k_score64, the components of its reach window
// plus the wide list -- ~2 sigma_min / (range / M) components instead of M --
// and every component when it lies off the planned range.
//
// Coherence: a block sorts its kP64N candidates by coordinate in LDS (bitonic)
// and each wave scores runs of 64 consecutive ones, looping over the union of
// its lanes' windows with wave-uniform (scalar) component loads; a lane adds
// only the components of its own window, so a candidate's sum -- terms, order
// and offset -- is a function of its coordinate alone, whatever its
// neighbours.  The offset is the mixture's largest log-coefficient (every
// term <= 1, one exp per pair); a sum below 2^-900 (or a candidate off the
// range, or NaN) is redone with the online log-sum-exp over all components.
#ifndef TPE_R64P  // diagnostic builds: candidates per thread of k_score_pruned64
#define TPE_R64P 8   // (2 048 sorted together: a wave's 64 span half the range of 4: fp64 C3 -10 %)
#endif
constexpr int kR64P = TPE_R64P;          // candidates per thread
constexpr int kP64N = kBS * kR64P;       // candidates per block (sorted together)

// exp(v) for the pruned sum's terms (v <= 0 or NaN; 0 below -745.2): n =
// rint(32 v / ln2), r = v - n ln2/32 (Cody-Waite, the high part's 32 bits
// keep n ln2_hi exact), exp(r) by its degree-6 Taylor polynomial (|r| <=
// ln2/64: truncation < 2^-57), times 2^((n mod 32)/32) from a 32-entry table
// (correctly rounded) and 2^(n div 32) -- within 3.25 * 2^-53 relative (three
// roundings, the truncation, the reduction), plus 2^-1074 where the result is
// subnormal; measured through tpe_exp_neg64_check on 1.26e6 arguments (every
// reduction tie among them): at most 1.93 ulp of the result (2.73 * 2^-53
// relative) on normal results, one unit of 2^-1074 on subnormal ones -- a
// sum of such terms keeps the scorer's 1e-13 -- with 13 instead of 17
// dependent fp64 steps and no overflow branch (round 6, with 2 048
// candidates per block: fp64 C3 level 256 -> 217 ms, same-box A/B)
__constant__ double kExp2Tab[32] = {
    0x1.0000000000000p+0, 0x1.059b0d3158574p+0, 0x1.0b5586cf9890fp+0, 0x1.11301d0125b51p+0,
    0x1.172b83c7d517bp+0, 0x1.1d4873168b9aap+0, 0x1.2387a6e756238p+0, 0x1.29e9df51fdee1p+0,
    0x1.306fe0a31b715p+0, 0x1.371a7373aa9cbp+0, 0x1.3dea64c123422p+0, 0x1.44e086061892dp+0,
    0x1.4bfdad5362a27p+0, 0x1.5342b569d4f82p+0, 0x1.5ab07dd485429p+0, 0x1.6247eb03a5585p+0,
    0x1.6a09e667f3bcdp+0, 0x1.71f75e8ec5f74p+0, 0x1.7a11473eb0187p+0, 0x1.82589994cce13p+0,
    0x1.8ace5422aa0dbp+0, 0x1.93737b0cdc5e5p+0, 0x1.9c49182a3f090p+0, 0x1.a5503b23e255dp+0,
    0x1.ae89f995ad3adp+0, 0x1.b7f76f2fb5e47p+0, 0x1.c199bdd85529cp+0, 0x1.cb720dcef9069p+0,
    0x1.d5818dcfba487p+0, 0x1.dfc97337b9b5fp+0, 0x1.ea4afa2a490dap+0, 0x1.f50765b6e4540p+0};
__device__ __forceinline__ double exp_neg64(double v, const double* __restrict__ tab) {
  const double n = rint(v * 0x1.71547652b82fep+5);
  double r = fma(-n, 0x1.62e42fee00000p-6, v);
  r = fma(-n, 0x1.a39ef35793c76p-38, r);
  double p = fma(r, 1.0 / 720.0, 1.0 / 120.0);
  p = fma(r, p, 1.0 / 24.0);
  p = fma(r, p, 1.0 / 6.0);
  p = fma(r, p, 0.5);
  p = fma(r, p, 1.0);
  p = fma(r, p, 1.0);
  const int ni = (int)fmax(n, -40000.0);  // (NaN: the polynomial is NaN already)
  const double e = ldexp(tab[ni & 31] * p, ni >> 5);
  return v < -745.2 ? 0.0 : e;
}

// largest log-coefficient of mixture S (every thread gets it)
__device__ __forceinline__ double lc_max(const tpe_seg& S, const double* __restrict__ coef64,
                                         double* red) {
  double m = -INFINITY;
  for (int k = threadIdx.x; k < S.n_obs + 1; k += kBS) m = fmax(m, coef64[4 * (S.comp_off + k) + 2]);
  return block_max<kBS, double>(m, red);
}

// log of mixture S at y for lane-active candidates (see above); call by the
// whole wave
__device__ __forceinline__ double lse64_pruned(const tpe_seg& S, const double* __restrict__ coef64,
                                               const double* __restrict__ rh,
                                               const double* __restrict__ rl,
                                               const int32_t* __restrict__ wide, int n_wide,
                                               double m, bool act, bool inr, double y,
                                               double4* stage, const double* etab) {
  const int nc = S.n_obs + 1;
  const int64_t off = S.comp_off;
  int k_lo = nc, k_hi = -1;
  if (act && inr) {
    k_lo = first_ge(rh + off, nc, y);
    k_hi = last_le(rl + off, nc, y);
  }
  const int ulo = wave_min_i(k_lo), uhi = wave_max_i(k_hi);
  double s = 0.0;
  // the union window in chunks of 64 components: one coalesced load per lane
  // into the wave's LDS slice (the wide flag folded in as w = 0), then every
  // lane reads the chunk's components in order by LDS broadcast -- the same
  // terms added in the same order as a loop over the window with a scalar
  // load per component (round 6: that loop waited on two dependent scalar
  // loads per component), so the sums are the same bits
  // (staged: x = mu, y = 1/sigma, z = log-coefficient - m, or -inf for a
  // component of the wide list -- its term is then exactly 0, and the wide
  // loop below adds it; the lane's own window as one unsigned compare)
  const int lane = lane_id();
  // (k_hi < k_lo, no window: a base no k reaches; uint32 arithmetic wraps)
  const uint32_t wlo = k_hi < k_lo ? 0x80000000u : (uint32_t)k_lo;
  const uint32_t wspan = k_hi < k_lo ? 0u : (uint32_t)(k_hi - k_lo);
  for (int kb = ulo; kb <= uhi; kb += kWave) {  // wave-uniform
    const int kk = kb + lane;
    double4 c = make_double4(0.0, 0.0, -INFINITY, 0.0);
    if (kk <= uhi) {
      c = ld4(coef64, off + kk);
      c.z = is_wide(S, kk, c.y) ? -INFINITY : c.z - m;
    }
    stage[lane] = c;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int n = min(kWave, uhi - kb + 1);
#pragma unroll 2
    for (int j = 0; j < n; ++j) {
      const double4 cj = stage[j];
      const double t = (y - cj.x) * cj.y;
      const double e = exp_neg64(fma(-0.5 * t, t, cj.z), etab);
      s += ((uint32_t)(kb + j) - wlo <= wspan) ? e : 0.0;
    }
    __builtin_amdgcn_wave_barrier();  // (the chunk read before the next one is staged)
  }
  if (__any(act && inr)) {
    for (int i = 0; i < n_wide; ++i) {
      const double4 c = ld4(coef64, off + wide[off + i]);
      const double t = (y - c.x) * c.y;
      s += exp(fma(-0.5 * t, t, c.z - m));
    }
  }
  double r = log(s) + m;
  const bool slow = act && !(inr && s >= 0x1p-900);
  if (__any(slow)) {
    // one exp per pair on every lane (as k_score64): same values as
    // s*exp(m-v)+1 (new max) / s+exp(v-m), NaN included
    double mo = -INFINITY, so = 0.0;
    for (int k = 0; k < nc; ++k) {
      const double4 c = ld4(coef64, off + k);
      const double t = (y - c.x) * c.y;
      const double v = -0.5 * (t * t) + c.z;
      const bool up = v > mo;
      const double e = exp(up ? mo - v : v - mo);
      so = up ? so * e + 1.0 : so + e;
      mo = up ? v : mo;
    }
    if (slow) r = log(so) + mo;
  }
  return r;
}

// ascending bitonic sort of kP64N (key, index) pairs in LDS, ties by index
__device__ __forceinline__ void sort_block(double* key, uint16_t* idx) {
  for (int k = 2; k <= kP64N; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
      for (int h = 0; h < kP64N / 2 / kBS; ++h) {
        const int p = h * kBS + threadIdx.x;
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i + j;
        const double a = key[i], b = key[l];
        const uint16_t ia = idx[i], ib = idx[l];
        const bool gt = a > b || (!(a < b) && ia > ib);
        if (gt == ((i & k) == 0)) {
          key[i] = b;
          key[l] = a;
          idx[i] = ib;
          idx[l] = ia;
        }
      }
      __syncthreads();
    }
  }
}

template <bool INJ>
__global__ __launch_bounds__(kBS) void k_score_pruned64(
    const tpe_job* __restrict__ jobs, const tpe_seg* __restrict__ segs,
    const double* __restrict__ mu, const double* __restrict__ sigma,
    const double* __restrict__ wcdf, const double* __restrict__ coef64,
    const double* __restrict__ reach_hi, const double* __restrict__ reach_lo,
    const int32_t* __restrict__ wide_idx, const tpe_table* __restrict__ tables,
    const double* __restrict__ cand, double* __restrict__ out_bl, double* __restrict__ out_al,
    double* __restrict__ out_x, tpe_best* __restrict__ partial) {
  __shared__ MixLds s_mix;
  __shared__ BestT red[kBS / kWave];
  __shared__ double dred[kBS / kWave];
  __shared__ double s_key[kP64N], s_x[kP64N];
  __shared__ uint16_t s_idx[kP64N];
  __shared__ double4 s_win[kBS / kWave][kWave];  // each wave's chunk of its union window
  __shared__ double s_etab[32];
  if (threadIdx.x < 32) s_etab[threadIdx.x] = kExp2Tab[threadIdx.x];  // (before the sort's barriers)
  const tpe_job J = jobs[blockIdx.y];
  tpe_best* P = partial + (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kP64N;
  if (base >= J.n_cand) {
    if (threadIdx.x == 0) *P = empty_best();
    return;
  }
  const int n_here = (int)min((int64_t)kP64N, J.n_cand - base);
  const tpe_seg SB = segs[J.below], SA = segs[J.above];
  const tpe_table Tb = tables[blockIdx.y];
  const bool lgmm = J.family == TPE_LGMM1;
  const bool lo_on = J.flags & TPE_F_LOW, hi_on = J.flags & TPE_F_HIGH;
  Mix M{};
  if (!INJ) M = stage_mix(SB, wcdf, mu, sigma, s_mix);
  for (int r = 0; r < kR64P; ++r) {
    const int i = r * kBS + threadIdx.x;
    double x = 0.0, y = INFINITY;
    if (i < n_here) {
      const int64_t li = base + i;
      if (INJ) {
        x = cand[J.cand_off + li];
        y = lgmm ? log(x) : x;
      } else if (J.flags & TPE_F_DRAW32) {
        // the table path's fp32 stream (the exact re-score of an overflowed band)
        const float y32 = draw32(M, J.key, J.cand_base + li, lo_on, hi_on, bound32(J.low),
                                 bound32(J.high));
        x = cand_value(y32, lgmm);
        y = score_coord(y32, lgmm);  // (LGMM1: log of the returned value, as INJ)
      } else {
        x = draw64(M, J.key, J.cand_base + li, lo_on, hi_on, J.low, J.high);
        if (lgmm) x = exp(x);
        y = lgmm ? log(x) : x;
      }
    }
    s_key[i] = y;
    s_x[i] = x;
    s_idx[i] = (uint16_t)i;
  }
  const double mb = lc_max(SB, coef64, dred), ma = lc_max(SA, coef64, dred);
  __syncthreads();
  sort_block(s_key, s_idx);
  BestT b{0.0, -1, 0.0};
  const int wid = threadIdx.x / kWave;
  for (int r = 0; r < kR64P; ++r) {
    const int p = (wid * kR64P + r) * kWave + lane_id();
    const int i = s_idx[p];
    const bool act = i < n_here;
    const double y = s_key[p], x = s_x[i];
    const bool inr = y >= Tb.lo && y <= Tb.hi;
    double bl = lse64_pruned(SB, coef64, reach_hi, reach_lo, wide_idx, Tb.n_wide_below, mb, act,
                             inr, y, s_win[wid], s_etab);
    double al = lse64_pruned(SA, coef64, reach_hi, reach_lo, wide_idx, Tb.n_wide_above, ma, act,
                             inr, y, s_win[wid], s_etab);
    if (!act) continue;
    if (lgmm) {  // lognormal_lpdf's -log(x) (tpe.py:214-216)
      bl -= y;
      al -= y;
    }
    const int64_t li = base + i;
    const int64_t o = J.out_off + li;
    if (out_bl) out_bl[o] = bl;
    if (out_al) out_al[o] = al;
    if (out_x) out_x[o] = x;
    best_update(b, bl - al, J.cand_base + li, x);
  }
  b = block_best<kBS>(b, red);
  if (threadIdx.x == 0) *P = tpe_best{b.score, b.index, b.value, 0};
}

// exp_neg64 on a caller's arguments (tpe_exp_neg64_check: the table staged in
// LDS as k_score_pruned64 stages it)
__global__ __launch_bounds__(kBS) void k_exp_neg64_check(const double* __restrict__ v, int64_t n,
                                                         double* __restrict__ out) {
  __shared__ double s_etab[32];
  if (threadIdx.x < 32) s_etab[threadIdx.x] = kExp2Tab[threadIdx.x];
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * kBS;
  for (int64_t i = (int64_t)blockIdx.x * kBS + threadIdx.x; i < n; i += stride)
    out[i] = exp_neg64(v[i], s_etab);
}
}  // namespace
}  // namespace tpe

using namespace tpe;

extern "C" int tpe_exp_neg64_check(const double* v, int64_t n, double* out, void* stream) {
  if (n < 0 || (n > 0 && (!v || !out))) {
    set_error("tpe_exp_neg64_check: bad arguments (n=%lld)", (long long)n);
    return TPE_E_ARG;
  }
  if (n == 0) return TPE_OK;
  const int64_t blocks = (n + kBS - 1) / kBS;
  hipLaunchKernelGGL(k_exp_neg64_check, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(kBS),
                     0, (hipStream_t)stream, v, n, out);
  return check_launch("tpe_exp_neg64_check");
}

extern "C" int64_t tpe_pruned64_partials(const tpe_job* host_jobs, int n_jobs) {
  return tiles_per_job(host_jobs, n_jobs, kP64N) * n_jobs;
}

extern "C" int tpe_score_pruned64(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                                  const tpe_seg* segs, const double* mu, const double* sigma,
                                  const double* wcdf, const double* coef64, int max_comp,
                                  double* reach_hi, double* reach_lo, int32_t* wide_idx,
                                  double* scratch, tpe_table* tables, const double* cand,
                                  double* out_bl, double* out_al, double* out_x,
                                  tpe_best* partial, int64_t n_partial, tpe_best* best,
                                  void* stream) {
  bool inj = false;
  if (!check_gmm_jobs("tpe_score_pruned64", host_jobs, n_jobs, 32767, 0, &inj)) return TPE_E_ARG;
  if (n_jobs == 0) return TPE_OK;
  if (!jobs || !segs || !mu || !sigma || !wcdf || !coef64 || !reach_hi || !reach_lo ||
      !wide_idx || !scratch || !tables || !partial || !best || (inj && !cand) || max_comp < 1) {
    set_error("tpe_score_pruned64: null pointer or max_comp < 1");
    return TPE_E_ARG;
  }
  const int64_t gx = tiles_per_job(host_jobs, n_jobs, kP64N);
  if (!check_partials("tpe_score_pruned64", n_partial, gx * n_jobs)) return TPE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  launch_table_plan(jobs, n_jobs, segs, mu, sigma, coef64, max_comp, reach_hi, reach_lo, wide_idx,
                    scratch, tables, kDrawZ64, kTauExact, st);
  const dim3 grid((unsigned)gx, (unsigned)n_jobs);
  dispatch_bool(inj, [&](auto INJ) {
    hipLaunchKernelGGL(k_score_pruned64<decltype(INJ)::value>, grid, dim3(kBS), 0, st, jobs, segs,
                       mu, sigma, wcdf, coef64, reach_hi, reach_lo, wide_idx, tables, cand, out_bl,
                       out_al, out_x, partial);
  });
  launch_reduce(jobs, partial, gx, best, n_jobs, st);
  return check_launch("tpe_score_pruned64");
}
