// tpe_categorical.hip -- categorical labels: sampling, scoring and argmax.
//
// Replaces, per label:
//   categorical sampling           hyperopt/pyll/stochastic.py:119-158
//   categorical_lpdf               hyperopt/tpe.py:60-73
//   broadcast_best (argmax)        hyperopt/tpe.py:649-658
//
// Exports: tpe_categorical_partials, tpe_score_categorical,
// tpe_categorical_suggest.
#include <algorithm>

#include "tpe_common.hpp"
#include "tpe_sample.hpp"

namespace tpe {
namespace {
constexpr int kRC = 16;      // categorical candidates per thread
constexpr int kCatKey = 256;  // categories of the rank-key fast path (8-bit category field)

// Categorical draws (randint / categorical priors sampled from the below
// posterior, tpe.py:575-610): candidate g takes word (g & 3) of the Philox call
// at counter (g >> 2, attempt 0) -- four candidates per call -- and its
// category is the first k with word < thr[k], thr[k] = ceil(cdf[k] / cdf[K-1]
// * 2^32): the inverse CDF at 2^-32 resolution, the same rule as the
// continuous samplers' component choice.  A threshold saturates at kThrSat =
// 2^32 - 1, so that one word is below no threshold; it goes where 2^32 - 2
// goes, to the first category whose threshold saturates (cat_edge: its
// interval ends at 2^32).  That category has mass; the ones after it -- a
// trailing category of probability zero, which hp.pchoice allows -- take no
// word at all.
constexpr uint32_t kThrSat = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t cat_thr(const double* cdf, int K, int k) {
  const double t = ceil(cdf[k] / cdf[K - 1] * 4294967296.0);
  return (t >= 4294967295.0) ? kThrSat : (t > 0.0 ? (uint32_t)t : 0u);
}
// end of category k's word interval [cat_edge(k - 1), cat_edge(k)); k = -1: 0
__device__ __forceinline__ uint64_t cat_edge(const double* cdf, int K, int k) {
  if (k < 0) return 0ull;
  const uint32_t t = cat_thr(cdf, K, k);
  return t == kThrSat ? (1ull << 32) : (uint64_t)t;
}
__device__ __forceinline__ int cat_search(const double* cdf, int K, uint32_t w) {
  w = min(w, kThrSat - 1u);
  int lo = 0, hi = K - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (w < cat_thr(cdf, K, mid)) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// injected candidates (given category indices): per-candidate lookup + argmax
__global__ __launch_bounds__(kBS) void k_score_cat_inj(
    const tpe_job* __restrict__ jobs, const tpe_cat_seg* __restrict__ csegs,
    const double* __restrict__ logp, const double* __restrict__ cand,
    double* __restrict__ out_bl, double* __restrict__ out_al, double* __restrict__ out_x,
    tpe_best* __restrict__ partial) {
  __shared__ BestT red[kBS / kWave];
  const tpe_job J = jobs[blockIdx.y];
  tpe_best* P = partial + (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  const int64_t base = (int64_t)blockIdx.x * (kBS * kRC);
  if (base >= J.n_cand) {
    if (threadIdx.x == 0) *P = empty_best();
    return;
  }
  const tpe_cat_seg CB = csegs[J.below], CA = csegs[J.above];
  const int K = CB.n_cat;
  const double* lb = logp + CB.p_off;
  const double* la = logp + CA.p_off;
  BestT b{0.0, -1, 0.0};
  for (int r = 0; r < kRC; ++r) {
    const int64_t li = base + r * kBS + threadIdx.x;
    if (li >= J.n_cand) break;
    const int64_t k = (int64_t)cand[J.cand_off + li];
    double bl = NAN, al = NAN;
    if (k >= 0 && k < K) {
      bl = lb[k];
      al = la[k];
    }
    const int64_t o = J.out_off + li;
    if (out_bl) out_bl[o] = bl;
    if (out_al) out_al[o] = al;
    if (out_x) out_x[o] = (double)k;
    best_update(b, bl - al, J.cand_base + li, (double)k);
  }
  b = block_best<kBS>(b, red);
  if (threadIdx.x == 0) *P = tpe_best{b.score, b.index, b.value, 0};
}

// sampled candidates.  The score depends on the category alone, so every
// category gets a rank (number of categories that beat it under np.argmax
// rules: NaN first, then larger score; equal scores share a rank) and a
// candidate's argmax key is rank << 48 | index << 8 | category: the smallest
// key is the reference's winner (best score, first index).  K <= KR: the
// thresholds sit in registers; KR < K <= kCatKey: binary search over the cdf
// (thresholds formed on the fly, same values); K > kCatKey: per-candidate
// fp64 argmax.  (The host picks KR from tpe_job.lat_n, the category count.)
__device__ __forceinline__ uint32_t word_of(const U4& q, int sel) {
  return sel == 0 ? q.x : sel == 1 ? q.y : sel == 2 ? q.z : q.w;
}

// Candidates [lo + blockIdx.x * kBS * kRC, ...) of job blockIdx.y; the
// block's winner goes to partial[job * nper + blockIdx.x].  need (nullable):
// jobs whose flag is 0 are skipped (the prefix-first path's second pass).
template <int KR>
__global__ __launch_bounds__(kBS) void k_score_cat(
    const tpe_job* __restrict__ jobs, const tpe_cat_seg* __restrict__ csegs,
    const double* __restrict__ logp, const double* __restrict__ cdf,
    double* __restrict__ out_bl, double* __restrict__ out_al, double* __restrict__ out_x,
    tpe_best* __restrict__ partial, int64_t lo, int64_t nper, const int32_t* __restrict__ need) {
  __shared__ double s_sc[kCatKey];
  __shared__ uint64_t s_key[kCatKey];
  __shared__ uint32_t s_thr[KR];
  __shared__ uint64_t red[kBS / kWave];
  if (need && !need[blockIdx.y]) return;  // block-uniform
  const tpe_job J = jobs[blockIdx.y];
  tpe_best* P = partial + (int64_t)blockIdx.y * nper + blockIdx.x;
  const int64_t base = lo + (int64_t)blockIdx.x * (kBS * kRC);
  if (base >= J.n_cand) {
    if (threadIdx.x == 0) *P = empty_best();
    return;
  }
  const tpe_cat_seg CB = csegs[J.below], CA = csegs[J.above];
  const int K = CB.n_cat;
  const double* lb = logp + CB.p_off;
  const double* la = logp + CA.p_off;
  const double* cb = cdf + CB.p_off;
  const int64_t t0 = base + (int64_t)threadIdx.x * kRC;
  const bool outs = out_bl || out_al || out_x;
  auto put = [&](int64_t li, int k) __attribute__((always_inline)) {
    if (outs) {
      const int64_t o = J.out_off + li;
      if (out_bl) out_bl[o] = lb[k];
      if (out_al) out_al[o] = la[k];
      if (out_x) out_x[o] = (double)k;
    }
  };
  if (K > kCatKey) {  // block-uniform: many categories, plain fp64 argmax
    BestT b{0.0, -1, 0.0};
    for (int r = 0; r < kRC; ++r) {
      const int64_t li = t0 + r;
      if (li >= J.n_cand) break;
      const int64_t g = J.cand_base + li;
      const int k = cat_search(cb, K, word_of(draw_words(J.key, g >> 2, 0, kStreamSample),
                                              (int)(g & 3)));
      put(li, k);
      best_update(b, lb[k] - la[k], g, (double)k);
    }
    b = block_best<kBS>(b, reinterpret_cast<BestT*>(s_sc));
    if (threadIdx.x == 0) *P = tpe_best{b.score, b.index, b.value, 0};
    return;
  }
  for (int k = threadIdx.x; k < K; k += kBS) {
    s_sc[k] = lb[k] - la[k];
    if (k < KR) s_thr[k] = cat_thr(cb, K, k);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += kBS) {
    const double sk = s_sc[k];
    uint32_t rank = 0;
    for (int j = 0; j < K; ++j) {
      const double sj = s_sc[j];
      rank += (sj != sj) ? (sk == sk) : (sk == sk && sj > sk);
    }
    s_key[k] = ((uint64_t)rank << 48) | (uint64_t)k;
  }
  __syncthreads();
  const bool in_regs = K <= KR;  // block-uniform
  uint32_t thr[KR - 1];
  int klast = 0;  // the first category whose threshold saturates (at most K - 1)
#pragma unroll
  for (int j = 0; j + 1 < KR; ++j) {
    thr[j] = (in_regs && j + 1 < K) ? s_thr[j] : kThrSat;
    klast += (thr[j] != kThrSat) ? 1 : 0;
  }
  auto category = [&](uint32_t w) __attribute__((always_inline)) -> int {
    if (in_regs) {
      int k = 0;
#pragma unroll
      for (int j = 0; j + 1 < KR; ++j) k += (w >= thr[j]) ? 1 : 0;
      return min(k, klast);  // (k > klast for the word 2^32 - 1 alone)
    }
    return cat_search(cb, K, w);
  };
  uint64_t best = ~0ull;
  auto take = [&](int64_t li, uint32_t w) __attribute__((always_inline)) {
    const int k = category(w);
    const int64_t g = J.cand_base + li;
    best = min(best, s_key[k] | ((uint64_t)g << 8));
    put(li, k);
  };
  const int64_t g0 = J.cand_base + t0;
  if ((g0 & 3) == 0 && t0 + kRC <= J.n_cand) {  // four candidates per Philox call
#pragma unroll
    for (int c = 0; c < kRC / 4; ++c) {
      const U4 r = draw_words(J.key, (g0 >> 2) + c, 0, kStreamSample);
      take(t0 + 4 * c + 0, r.x);
      take(t0 + 4 * c + 1, r.y);
      take(t0 + 4 * c + 2, r.z);
      take(t0 + 4 * c + 3, r.w);
    }
  } else {  // unaligned base or the job's last candidates: one call per candidate
    for (int r = 0; r < kRC; ++r) {
      const int64_t li = t0 + r;
      if (li >= J.n_cand) break;
      const int64_t g = J.cand_base + li;
      take(li, word_of(draw_words(J.key, g >> 2, 0, kStreamSample), (int)(g & 3)));
    }
  }
  // block min of the keys
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint64_t o = __shfl_xor(best, off, kWave);
    best = min(best, o);
  }
  if (lane_id() == 0) red[threadIdx.x / kWave] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t b = red[0];
#pragma unroll
    for (int w = 1; w < kBS / kWave; ++w) b = min(b, red[w]);
    if (b == ~0ull) {
      *P = empty_best();
    } else {
      const int k = (int)(b & 0xFF);
      const int64_t g = (int64_t)((b >> 8) & ((1ull << 40) - 1));
      *P = tpe_best{s_sc[k], g, (double)k, 0};
    }
  }
}

// The prefix-first decision for categorical jobs (tpe_categorical_suggest).
// Pass 0: the winner of the first `prefix` candidates (partials [0, n1)); a
// later candidate can only beat it with a strictly better score (its index is
// larger), i.e. with a category that scores better -- and every such category
// is absent from the prefix (else it would have won there).  need[j] = 1 when
// one of them can be drawn at all (a non-empty inverse-CDF interval) and the
// stream is longer than the prefix.  Pass 1 (jobs with need): the rest's
// partials [0, n2) folded into best[j].
__global__ __launch_bounds__(kBS) void k_cat_decide(
    const tpe_job* __restrict__ jobs, const tpe_cat_seg* __restrict__ csegs,
    const double* __restrict__ logp, const double* __restrict__ cdf,
    const tpe_best* __restrict__ partial, int64_t nper, int64_t n_use, int64_t prefix, int pass,
    int32_t* __restrict__ need, tpe_best* __restrict__ best) {
  __shared__ BestT red[kBS / kWave];
  const int j = blockIdx.x;
  if (pass == 1 && !need[j]) return;  // block-uniform
  const tpe_job J = jobs[j];
  const tpe_best* P = partial + (int64_t)j * nper;
  BestT b{0.0, -1, 0.0};
  if (pass == 1 && threadIdx.x == 0) b = BestT{best[j].score, best[j].index, best[j].value};
  for (int64_t i = threadIdx.x; i < n_use; i += kBS) best_update(b, P[i].score, P[i].index, P[i].value);
  b = block_best<kBS>(b, red);
  int open = 0;
  if (pass == 0 && J.n_cand > prefix) {
    const tpe_cat_seg CB = csegs[J.below], CA = csegs[J.above];
    const int K = CB.n_cat;
    for (int k = threadIdx.x; k < K && !open; k += kBS) {
      const double sk = logp[CB.p_off + k] - logp[CA.p_off + k];
      // category k takes the words [cat_edge(k - 1), cat_edge(k)): none when it
      // has no mass, a trailing category included
      const uint64_t t0 = cat_edge(cdf + CB.p_off, K, k - 1);
      const uint64_t t1 = cat_edge(cdf + CB.p_off, K, k);
      open = better(sk, INT64_MAX, b.score, b.index) && t1 > t0;
    }
    open = __syncthreads_or(open);
  }
  if (threadIdx.x == 0) {
    best[j] = tpe_best{b.score, b.index, b.value, J.n_cand};
    if (pass == 0) need[j] = open;
  }
}
}  // namespace
}  // namespace tpe

using namespace tpe;

// k_score_cat for the launch's largest category count (tpe_job.lat_n of
// categorical jobs; 0 = unknown)
static void launch_cat(const tpe_job* host_jobs, int n_jobs, dim3 grid, hipStream_t st,
                       const tpe_job* jobs, const tpe_cat_seg* csegs, const double* logp,
                       const double* cdf, double* out_bl, double* out_al, double* out_x,
                       tpe_best* partial, int64_t lo, int64_t nper, const int32_t* need) {
  int kmax = 1;
  for (int i = 0; i < n_jobs; ++i)
    kmax = std::max(kmax, host_jobs[i].lat_n > 0 ? (int)host_jobs[i].lat_n : kCatKey);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(kBS), 0, st, jobs, csegs, logp, cdf, out_bl, out_al,
                       out_x, partial, lo, nper, need);
  };
  if (kmax <= 4)
    launch(k_score_cat<4>);
  else if (kmax <= 8)
    launch(k_score_cat<8>);
  else
    launch(k_score_cat<16>);
}

extern "C" int64_t tpe_categorical_partials(const tpe_job* host_jobs, int n_jobs) {
  return (int64_t)n_jobs * tiles_per_job(host_jobs, n_jobs, kBS * kRC);
}

extern "C" int tpe_score_categorical(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                                     const tpe_cat_seg* csegs, const double* logp_pool,
                                     const double* cdf_pool, const double* cand,
                                     double* out_bl, double* out_al, double* out_x,
                                     tpe_best* partial, int64_t n_partial, tpe_best* best,
                                     void* stream) {
  if (!check_jobs("tpe_score_categorical", host_jobs, n_jobs)) return TPE_E_ARG;
  if (n_jobs == 0) return TPE_OK;
  bool inj = false;
  for (int i = 0; i < n_jobs; ++i) {
    if (host_jobs[i].family != TPE_CAT) {
      set_error("tpe_score_categorical: job %d is not categorical", i);
      return TPE_E_ARG;
    }
    const bool ji = (host_jobs[i].flags & TPE_F_INJECTED) != 0;
    if (i > 0 && ji != inj) {
      set_error("tpe_score_categorical: mixed injected / sampled jobs in one call");
      return TPE_E_ARG;
    }
    inj = ji;
  }
  if (!jobs || !csegs || !logp_pool || !cdf_pool || !partial || !best || (inj && !cand)) {
    set_error("tpe_score_categorical: null pointer");
    return TPE_E_ARG;
  }
  const int64_t gx = tiles_per_job(host_jobs, n_jobs, (int64_t)kBS * kRC);
  if (gx * n_jobs > n_partial) {
    set_error("tpe_score_categorical: partial workspace too small");
    return TPE_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)gx, (unsigned)n_jobs);
  if (inj)
    hipLaunchKernelGGL(k_score_cat_inj, grid, dim3(kBS), 0, st, jobs, csegs, logp_pool, cand,
                       out_bl, out_al, out_x, partial);
  else
    launch_cat(host_jobs, n_jobs, grid, st, jobs, csegs, logp_pool, cdf_pool, out_bl, out_al,
               out_x, partial, 0, gx, nullptr);
  launch_reduce(jobs, partial, gx, best, n_jobs, st);
  return check_launch("tpe_score_categorical");
}

// prefix-first categorical argmax (the suggest path; see k_cat_decide)
extern "C" int tpe_categorical_suggest(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                                       const tpe_cat_seg* csegs, const double* logp_pool,
                                       const double* cdf_pool, int64_t prefix, tpe_best* partial,
                                       int64_t n_partial, int32_t* need, tpe_best* best,
                                       void* stream) {
  if (!check_jobs("tpe_categorical_suggest", host_jobs, n_jobs)) return TPE_E_ARG;
  if (n_jobs == 0) return TPE_OK;
  for (int i = 0; i < n_jobs; ++i)
    if (host_jobs[i].family != TPE_CAT || (host_jobs[i].flags & TPE_F_INJECTED)) {
      set_error("tpe_categorical_suggest: job %d is not a sampled categorical job", i);
      return TPE_E_ARG;
    }
  if (!jobs || !csegs || !logp_pool || !cdf_pool || !partial || !need || !best) {
    set_error("tpe_categorical_suggest: null pointer");
    return TPE_E_ARG;
  }
  constexpr int64_t kT = (int64_t)kBS * kRC;
  if (prefix <= 0 || prefix % kT != 0) {
    set_error("tpe_categorical_suggest: prefix %lld is not a positive multiple of %lld",
              (long long)prefix, (long long)kT);
    return TPE_E_ARG;
  }
  const int64_t gx = tiles_per_job(host_jobs, n_jobs, kT);
  if (!check_partials("tpe_categorical_suggest", n_partial, gx * n_jobs)) return TPE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int64_t g1 = std::min(gx, prefix / kT);  // prefix blocks per job
  launch_cat(host_jobs, n_jobs, dim3((unsigned)g1, (unsigned)n_jobs), st, jobs, csegs, logp_pool,
             cdf_pool, nullptr, nullptr, nullptr, partial, 0, gx, nullptr);
  hipLaunchKernelGGL(k_cat_decide, dim3(n_jobs), dim3(kBS), 0, st, jobs, csegs, logp_pool,
                     cdf_pool, partial, gx, g1, prefix, 0, need, best);
  if (gx > g1) {  // the rest of the streams that need it (blocks of the others exit at once)
    launch_cat(host_jobs, n_jobs, dim3((unsigned)(gx - g1), (unsigned)n_jobs), st, jobs, csegs,
               logp_pool, cdf_pool, nullptr, nullptr, nullptr, partial, prefix, gx, need);
    hipLaunchKernelGGL(k_cat_decide, dim3(n_jobs), dim3(kBS), 0, st, jobs, csegs, logp_pool,
                       cdf_pool, partial, gx, gx - g1, prefix, 1, need, best);
  }
  return check_launch("tpe_categorical_suggest");
}
