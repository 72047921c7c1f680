// tpe_quantized.hip -- quantized continuous labels: the lattice path.
//
// Replaces the q-rounded GMM1 / LGMM1 sampling (hyperopt/tpe.py:79-106,
// 229-257), their erf-pair log-mass (tpe.py:159-174, 288-305) and the argmax
// of broadcast_best (tpe.py:649-658).  Candidate values are k*q, so each
// distinct value is scored once in fp64 with the reference's erf-pair sum and
// the argmax keeps the first candidate index of the best value.
//
// Exports: tpe_lattice_sample, tpe_lattice_suggest, tpe_lattice_compact,
// tpe_quantized_partials, tpe_score_quantized.
#include <algorithm>

#include "tpe_common.hpp"
#include "tpe_sample.hpp"

namespace tpe {
namespace {
constexpr int kLatLds = 4096;  // lattice slots deduplicated in LDS per block

// POW2: every job draws in fp32 (TPE_F_DRAW32) with q a power of two and at
// most kLatLds lattice slots (C3's quniform labels) -- slots come from rintf
// in fp32 and the kernel carries no fp64 slot code (fewer registers); the
// general instantiation handles the rest.  lfirst is dynamic LDS sized by the
// host to the largest lattice of the launch (up to kLatLds slots).
__host__ __device__ __forceinline__ bool lattice_pow2(const tpe_job& j) {
  int qe;
  return (j.flags & TPE_F_DRAW32) && frexp(j.q, &qe) == 0.5 && qe > -100 && qe < 100 &&
         j.lat_n <= kLatLds;
}

// Component windows of the quantized log-mass (round 5).  A component whose
// two erf arguments are both beyond +-6.5 contributes exactly 0 (qlpdf skips
// it), i.e. unless mu - b < ub and mu + b > lb, b = 6.5 max(sqrt2 sigma, EPS).
// The means are sorted, so with P[k] = max_{j<=k} (mu_j + b_j) and
// S[k] = min_{j>=k} (mu_j - b_j) (both non-decreasing; k_qreach) every
// component that can contribute lies in [first k with P[k] > lb, last k with
// S[k] < ub] -- found by a block-wide search -- and qlpdf loops over that
// window only.  Each thread still visits its own components in the same
// order and skips the same ones, so the sums are bit-identical to the full
// loop's.  A NaN mean or sigma gives P = +inf / S = -inf from there on, which
// keeps NaN components (sorted last) inside every window.
constexpr int kQB = 256;  // k_qreach block: one per segment (small: it runs beside the table build)
constexpr int kQPer = 8;   // components per thread per pass (all its loads issued together)
__device__ __forceinline__ double qreach_b(double s) { return 6.5 * fmax(__dmul_rn(kSqrt2, s), kEps); }


// One block per (job, mixture, direction): blockIdx.x = 4 job + 2 dir + mix,
// dir 0 the prefix max P from the front, dir 1 the suffix min S from the
// back; the next pass's loads are issued before this pass's scan (the block
// walks ~50 passes of 2 048 components at C5's 10^5: each otherwise waited
// one load round trip)
__global__ __launch_bounds__(kQB) void k_qreach(const tpe_job* __restrict__ jobs,
                                               const tpe_seg* __restrict__ segs,
                                               const double* __restrict__ mu,
                                               const double* __restrict__ sigma,
                                               double* __restrict__ P, double* __restrict__ Sm) {
  __shared__ double sw[kQB / kWave];
  const tpe_job J = jobs[blockIdx.x >> 2];
  const bool suffix = (blockIdx.x >> 1) & 1;
  const tpe_seg S = segs[(blockIdx.x & 1) ? J.above : J.below];
  const int nc = S.n_obs + 1;
  const double* m = mu + S.comp_off;
  const double* g = sigma + S.comp_off;
  constexpr int kPass = kQB * kQPer;
  const int npass = (nc + kPass - 1) / kPass;
  // thread t's raw loads of components base + t * kQPer + i
  auto load = [&](int base, double (&mk)[kQPer], double (&gk)[kQPer]) __attribute__((always_inline)) {
    const int a = base + (int)threadIdx.x * kQPer;
#pragma unroll
    for (int i = 0; i < kQPer; ++i) {
      const int k = a + i;
      mk[i] = k < nc ? m[k] : 0.0;
      gk[i] = k < nc ? g[k] : 0.0;
    }
  };
  // (hi = mu + b for the prefix, lo = mu - b for the suffix; NaN -> +inf / -inf)
  auto value = [&](int k, double mk, double gk) -> double {
    const double r = qreach_b(gk);
    const bool ok = mk == mk && r == r;
    if (!suffix) return k >= nc ? -INFINITY : (ok ? mk + r : INFINITY);
    return k >= nc ? INFINITY : (ok ? mk - r : -INFINITY);
  };
  double nm[kQPer], ng[kQPer];
  load(suffix ? (npass - 1) * kPass : 0, nm, ng);
  double carry = suffix ? INFINITY : -INFINITY;  // the earlier passes' max / later passes' min
  for (int q = 0; q < npass; ++q) {  // block-uniform
    const int ps = suffix ? npass - 1 - q : q;
    const int base = ps * kPass;
    const int a = base + (int)threadIdx.x * kQPer;
    double v[kQPer];
#pragma unroll
    for (int i = 0; i < kQPer; ++i) v[i] = value(a + i, nm[i], ng[i]);
    if (q + 1 < npass) load((suffix ? ps - 1 : ps + 1) * kPass, nm, ng);  // (in flight)
    if (!suffix) {
#pragma unroll
      for (int i = 1; i < kQPer; ++i) v[i] = fmax(v[i], v[i - 1]);
      const double incl = block_prefix_max(v[kQPer - 1], sw);
      double before = __shfl_up(incl, 1, kWave);  // max over the threads before this one
      if (lane_id() == 0) {
        before = -INFINITY;
        for (int w = 0; w < (int)threadIdx.x / kWave; ++w) before = fmax(before, sw[w]);
      }
      before = fmax(before, carry);
#pragma unroll
      for (int i = 0; i < kQPer; ++i)
        if (a + i < nc) P[S.comp_off + a + i] = fmax(before, v[i]);
      for (int w = 0; w < kQB / kWave; ++w) carry = fmax(carry, sw[w]);  // (the pass's total)
    } else {
#pragma unroll
      for (int i = kQPer - 2; i >= 0; --i) v[i] = fmin(v[i], v[i + 1]);
      const double incl = block_suffix_min<kQB>(v[0], sw);
      double after = __shfl_down(incl, 1, kWave);  // min over the threads after this one
      if (lane_id() == kWave - 1) {
        after = INFINITY;
        for (int w = (int)threadIdx.x / kWave + 1; w < kQB / kWave; ++w) after = fmin(after, sw[w]);
      }
      after = fmin(after, carry);
#pragma unroll
      for (int i = 0; i < kQPer; ++i)
        if (a + i < nc) Sm[S.comp_off + a + i] = fmin(after, v[i]);
      for (int w = 0; w < kQB / kWave; ++w) carry = fmin(carry, sw[w]);  // (the pass's total)
    }
    __syncthreads();
  }
}

// normal_cdf(x, m, s) (GMM1) or lognormal_cdf_logx(x = log of the bound, m,
// s) (LGMM1) with one erf: the two share z = (x - m) / max(sqrt2 s, EPS) and
// differ only in how erf(z) is combined (numpy's order for each: 0.5 * (1 +
// e), tpe.py:109-114; 0.5 + 0.5 * e, tpe.py:186-205) -- one inlined erf per
// bound instead of one per family and bound (register pressure)
__device__ __forceinline__ double qcdf(bool lg, double x, double m, double s) {
  const double bottom = fmax(__dmul_rn(kSqrt2, s), kEps);
  const double e = erf((x - m) / bottom);
  return lg ? __dadd_rn(0.5, __dmul_rn(0.5, e)) : __dmul_rn(0.5, __dadd_rn(1.0, e));
}

// quantized mixture log-mass of one value, one WAVE, lanes stride components
// (lane l takes components k = l mod 64, in order).  tpe.py:159-174 (GMM1) and
// :288-305 (LGMM1): sum_k w_k*cdf(ub) - w_k*cdf(lb), then log(prob) -
// log(p_accept).  P / Sm (nullable): k_qreach's arrays -- the loop then
// covers the value's component window only, entered at the full loop's pass
// that holds the window's first component, so every lane visits the same
// components in the same order and skips the same ones: the same sums, bit
// for bit.  The lanes' partial sums meet in one fixed butterfly.  Round 6: a
// wave per value instead of a 256-thread block (C4's ~370-component windows
// left a block's threads one or two components each, behind eight block-wide
// barriers per value).  Every lane returns the value.
__device__ __forceinline__ double qlpdf(const tpe_job& J, const tpe_seg& S,
                                        const double* __restrict__ w,
                                        const double* __restrict__ mu,
                                        const double* __restrict__ sigma, double x,
                                        int32_t* err,
                                        const double* __restrict__ P = nullptr,
                                        const double* __restrict__ Sm = nullptr) {
  const bool lg = J.family == TPE_LGMM1;
  const double hq = J.q / 2.0;
  double ub = x + hq, lb = x - hq;
  if (J.flags & TPE_F_HIGH) ub = fmin(ub, lg ? exp(J.high) : J.high);
  if (J.flags & TPE_F_LOW) lb = fmax(lb, lg ? exp(J.low) : J.low);
  double lub = 0.0, llb = 0.0;
  const int lane = lane_id();
  if (lg) {
    lb = fmax(0.0, lb);
    if (ub < 0.0 && lane == 0 && err) atomicOr(err, 1);  // tpe.py:196-197
    lub = log(ub < kEps ? kEps : ub);
    llb = log(lb < kEps ? kEps : lb);
  }
  const int nc = S.n_obs + 1;
  double acc = 0.0;
  const double xu = lg ? lub : ub, xl = lg ? llb : lb;
  // kQU components per lane per pass, their loads issued together
  constexpr int kQU = 4;
  constexpr int kPassQ = kQU * kWave;
  int kbeg = 0, kend = nc;
  const double dl = 1e-9 * (1.0 + fabs(xl) + fabs(xu));  // (covers the fp64 rounding of mu +- b)
  const double wa = xl - dl, wb = xu + dl;
  if (P && wa == wa && wb == wb) {  // wave-uniform
    kbeg = wave_prefix_count(nc, [&](int k) { return P[S.comp_off + k] <= wa; });
    kend = max(kbeg, wave_prefix_count(nc, [&](int k) { return Sm[S.comp_off + k] < wb; }));
  }
  for (int k0 = kbeg / kPassQ * kPassQ + lane; k0 < kend; k0 += kPassQ) {
    double mq[kQU], sq[kQU];
#pragma unroll
    for (int u = 0; u < kQU; ++u) {
      const int k = k0 + u * kWave;
      const bool in = k >= kbeg && k < kend;
      mq[u] = in ? mu[S.comp_off + k] : INFINITY;
      sq[u] = in ? sigma[S.comp_off + k] : 1.0;
    }
#pragma unroll
    for (int u = 0; u < kQU; ++u) {
      const double m = mq[u], s = sq[u];
      // both erf arguments beyond +-6.5 (erf exactly +-1 in fp64): the two cdf
      // values are equal and the term w*cu - w*cl is exactly 0 -- skip it
      // (padding: m = +inf is skipped)
      const double b65 = 6.5 * fmax(__dmul_rn(kSqrt2, s), kEps);
      if (xl - m >= b65 || xu - m <= -b65 || m == INFINITY) continue;
      const double wk = w[S.comp_off + k0 + u * kWave];
      const double cu = qcdf(lg, xu, m, s), cl = qcdf(lg, xl, m, s);
      acc += __dsub_rn(__dmul_rn(wk, cu), __dmul_rn(wk, cl));  // two-stage, as tpe.py:171-173
    }
  }
#pragma unroll
  for (int o = kWave / 2; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, kWave);
  return log(acc) - log(S.p_accept);
}

// The same log-mass with the whole BLOCK on one value (threads stride the
// components, k = t mod 256; block-wide window search and sum): for mixtures
// of more than kQBig components (C3's 10^4, C5's 10^5), whose windows give a wave
// thousands of CDF pairs.  Its own bits (another lane map), chosen per
// mixture size alone (qlpdf_big), so every kernel scoring a value picks the
// same variant.
__device__ __forceinline__ double qlpdf_block(const tpe_job& J, const tpe_seg& S,
                                        const double* __restrict__ w,
                                        const double* __restrict__ mu,
                                        const double* __restrict__ sigma, double x,
                                        int32_t* err, double* sh,
                                        const double* __restrict__ P = nullptr,
                                        const double* __restrict__ Sm = nullptr) {
  const bool lg = J.family == TPE_LGMM1;
  const double hq = J.q / 2.0;
  double ub = x + hq, lb = x - hq;
  if (J.flags & TPE_F_HIGH) ub = fmin(ub, lg ? exp(J.high) : J.high);
  if (J.flags & TPE_F_LOW) lb = fmax(lb, lg ? exp(J.low) : J.low);
  double lub = 0.0, llb = 0.0;
  if (lg) {
    lb = fmax(0.0, lb);
    if (ub < 0.0 && threadIdx.x == 0 && err) atomicOr(err, 1);  // tpe.py:196-197
    lub = log(ub < kEps ? kEps : ub);
    llb = log(lb < kEps ? kEps : lb);
  }
  const int nc = S.n_obs + 1;
  double acc = 0.0;
  const double xu = lg ? lub : ub, xl = lg ? llb : lb;
  // kQU components per thread per pass, their loads issued together (the
  // skip test is cheap; a serial load -> test chain per component is what
  // bounded this loop)
  constexpr int kQU = 4;
  int kbeg = 0, kend = nc;
  const double dl = 1e-9 * (1.0 + fabs(xl) + fabs(xu));  // (covers the fp64 rounding of mu +- b)
  const double wa = xl - dl, wb = xu + dl;
  if (P && wa == wa && wb == wb) {  // block-uniform
    kbeg = block_prefix_count<kBS>(nc, [&](int k) { return P[S.comp_off + k] <= wa; });
    kend = max(kbeg, block_prefix_count<kBS>(nc, [&](int k) { return Sm[S.comp_off + k] < wb; }));
  }
  // the full loop's thread-to-component map, entered at the window's first pass
  for (int k0 = kbeg / (kQU * kBS) * (kQU * kBS) + threadIdx.x; k0 < kend; k0 += kQU * kBS) {
    double mq[kQU], sq[kQU];
#pragma unroll
    for (int u = 0; u < kQU; ++u) {
      const int k = k0 + u * kBS;
      const bool in = k >= kbeg && k < kend;
      mq[u] = in ? mu[S.comp_off + k] : INFINITY;
      sq[u] = in ? sigma[S.comp_off + k] : 1.0;
    }
#pragma unroll
    for (int u = 0; u < kQU; ++u) {
      const double m = mq[u], s = sq[u];
      // both erf arguments beyond +-6.5 (erf exactly +-1 in fp64): the two cdf
      // values are equal and the term w*cu - w*cl is exactly 0 -- skip it
      // (padding: m = +inf is skipped)
      const double b65 = 6.5 * fmax(__dmul_rn(kSqrt2, s), kEps);
      if (xl - m >= b65 || xu - m <= -b65 || m == INFINITY) continue;
      const double wk = w[S.comp_off + k0 + u * kBS];
      const double cu = qcdf(lg, xu, m, s), cl = qcdf(lg, xl, m, s);
      acc += __dsub_rn(__dmul_rn(wk, cu), __dmul_rn(wk, cl));  // two-stage, as tpe.py:171-173
    }
  }
  acc = block_sum<kBS, double>(acc, sh);
  return log(acc) - log(S.p_accept);
}

// mixtures above this many components take the block-wide log-mass
constexpr int kQBig = 4096;
__device__ __forceinline__ bool qlpdf_big(const tpe_seg& SB, const tpe_seg& SA) {
  return max(SB.n_obs, SA.n_obs) + 1 > kQBig;
}

// one wave per value (kQW values per 256-thread block): the wave shares the
// value's component CDF pairs
constexpr int kQW = kBS / kWave;

// grid (nper, n_jobs), nper = the partial entries per job (>= every job's
// count): a job of small mixtures scores value pos = kQW blockIdx.x + wave,
// one of large ones (qlpdf_big) value blockIdx.x with the whole block
__global__ __launch_bounds__(kBS) void k_score_q(
    const tpe_job* __restrict__ jobs, const tpe_seg* __restrict__ segs,
    const double* __restrict__ w, const double* __restrict__ mu,
    const double* __restrict__ sigma, const double* __restrict__ vals,
    const int64_t* __restrict__ firsts, const unsigned long long* __restrict__ counts,
    double* __restrict__ out_bl, double* __restrict__ out_al, tpe_best* __restrict__ partial,
    int32_t* __restrict__ err, const double* __restrict__ qP, const double* __restrict__ qS,
    int64_t nper) {
  __shared__ double sh[kBS / kWave];
  const tpe_job J = jobs[blockIdx.y];
  const tpe_seg SB = segs[J.below], SA = segs[J.above];
  const int64_t cnt = counts ? (int64_t)counts[blockIdx.y] : J.n_cand;
  const int64_t voff = counts ? J.lat_off : J.cand_off;
  auto put = [&](int64_t pos, double bl, double al, double v) __attribute__((always_inline)) {
    const int64_t idx = firsts ? firsts[J.lat_off + pos] : J.cand_base + pos;
    if (out_bl) out_bl[J.out_off + pos] = bl;
    if (out_al) out_al[J.out_off + pos] = al;
    partial[(int64_t)blockIdx.y * nper + pos] = tpe_best{bl - al, idx, v, 0};
  };
  if (qlpdf_big(SB, SA)) {  // block-uniform: block b scores value b with every thread
    const int64_t pos = blockIdx.x;
    if (pos >= nper) return;
    if (pos >= cnt) {
      if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * nper + pos] = empty_best();
      return;
    }
    const double v = vals[voff + pos];
    const double bl = qlpdf_block(J, SB, w, mu, sigma, v, err, sh, qP, qS);
    const double al = qlpdf_block(J, SA, w, mu, sigma, v, err, sh, qP, qS);
    if (threadIdx.x == 0) put(pos, bl, al, v);
    return;
  }
  // otherwise block b < nper / kQW scores values kQW b .. one per wave (the
  // grid has a block per value for the large-mixture jobs; the rest exit)
  const int64_t pos = (int64_t)blockIdx.x * kQW + threadIdx.x / kWave;
  if (pos >= nper) return;  // wave-uniform
  const bool lead = lane_id() == 0;
  if (pos >= cnt) {  // wave-uniform
    if (lead) partial[(int64_t)blockIdx.y * nper + pos] = empty_best();
    return;
  }
  const double v = vals[voff + pos];
  const double bl = qlpdf(J, SB, w, mu, sigma, v, err, qP, qS);
  const double al = qlpdf(J, SA, w, mu, sigma, v, err, qP, qS);
  if (lead) put(pos, bl, al, v);
}

// Prefix-first lattice argmax (tpe_lattice_suggest).  A lattice value's score
// does not depend on where it is drawn, and the reference's winner is the
// best-scoring value that occurs in the stream, at its first occurrence
// (np.argmax: first index of the maximum).  So after the first `prefix`
// candidates the winner is settled unless some value not yet seen scores
// strictly higher (or is NaN while the best seen is not): a value first seen
// later has a larger index and loses every tie.  score_slots scores every
// slot of the lattice (seen or not), k_lattice_decide takes the argmax over
// the seen ones and flags the jobs where an unseen slot could still win; only
// those draw the rest of their stream (the sampler with `need`) and decide
// again over everything seen.  (The slots are scored by extra blocks of the
// prefix's sampling launch, k_lattice_sample.)
// Slot block sb of job `job` (slot_n blocks per job): slots
// kSlotsPerBlock sb .. one per wave, or (mixtures past kQBig, qlpdf_big)
// slot sb with the whole block; the blocks past a job's slots exit.  sh:
// kBS / kWave doubles of LDS.  Call by the whole block.
constexpr int kSlotsPerBlock = kBS / kWave;  // score_slots: lattice slots per block
__device__ __forceinline__ void score_slots(const tpe_job* __restrict__ jobs,
                                            const tpe_seg* __restrict__ segs,
                                            const double* __restrict__ w,
                                            const double* __restrict__ mu,
                                            const double* __restrict__ sigma,
                                            tpe_best* __restrict__ partial, int job, int64_t sb,
                                            int64_t nper, double* sh, const double* __restrict__ P,
                                            const double* __restrict__ Sm) {
  const tpe_job J = jobs[job];
  const tpe_seg SB = segs[J.below], SA = segs[J.above];
  // every slot is scored, drawn or not: a slot below 0 (the bracket under a
  // qloguniform / qlognormal lattice, never drawn) must not raise the
  // reference's negative-argument error (tpe.py:196-197) -- a drawn value
  // x = round(exp(y)/q)*q >= 0 never has ub = x + q/2 < 0, so no err here
  auto value = [&](int64_t s) { return (double)(J.lat_kmin + s) * J.q; };  // as k_lattice_compact
  if (qlpdf_big(SB, SA)) {  // block-uniform: slot sb with every thread
    const int64_t s = sb;
    if (s >= J.lat_n || s >= nper) return;
    const double v = value(s);
    const double bl = qlpdf_block(J, SB, w, mu, sigma, v, nullptr, sh, P, Sm);
    const double al = qlpdf_block(J, SA, w, mu, sigma, v, nullptr, sh, P, Sm);
    if (threadIdx.x == 0) partial[(int64_t)job * nper + s] = tpe_best{bl - al, -1, v, 0};
    return;
  }
  const int64_t s = sb * kSlotsPerBlock + threadIdx.x / kWave;
  if (s >= J.lat_n || s >= nper) return;  // wave-uniform
  const double v = value(s);
  const double bl = qlpdf(J, SB, w, mu, sigma, v, nullptr, P, Sm);
  const double al = qlpdf(J, SA, w, mu, sigma, v, nullptr, P, Sm);
  if (lane_id() == 0) partial[(int64_t)job * nper + s] = tpe_best{bl - al, -1, v, 0};
}

// Candidates [start, min(n_cand, limit)) of every job (start a multiple of the
// kBS * kLatR tile); need (nullable): only the jobs whose flag is set.
// slot_n > 0 (tpe_lattice_suggest's first launch): the grid's first
// slot_n * n_jobs blocks score the lattice slots instead (score_slots; the
// slot scores do not depend on the draws, so they share the launch)
template <bool POW2>
#ifndef TPE_LAT_WPE  // diagnostic builds: waves-per-EU target of the lattice sampler
#define TPE_LAT_WPE 4     // (power-of-two candidate counts: 128 VGPRs, no spill)
#endif
__global__ __launch_bounds__(kBS) __attribute__((amdgpu_waves_per_eu(POW2 ? TPE_LAT_WPE : 1))) void k_lattice_sample(
    const tpe_job* __restrict__ jobs, const tpe_seg* __restrict__ segs,
    const double* __restrict__ mu, const double* __restrict__ sigma,
    const double* __restrict__ wcdf, unsigned long long* __restrict__ slot_first,
    int32_t* __restrict__ err, int n_tiles, int n_jobs, int64_t start, int64_t limit,
    const int32_t* __restrict__ need, const double* __restrict__ w,
    tpe_best* __restrict__ slot_part, int slot_n, const double* __restrict__ qP,
    const double* __restrict__ qS) {
  extern __shared__ uint32_t lfirst[];
  __shared__ MixLds s_mix;
  __shared__ alignas(16) float s_stage[kLatR * kBS];  // (also the slot blocks' fp64 scratch)
  __shared__ uint16_t s_list[(kBS / kWave) * kRetryList];
  const int64_t spj = slot_n;  // slot blocks per job (score_slots)
  const int64_t slot_blocks = spj * n_jobs;
  if ((int64_t)blockIdx.x < slot_blocks) {  // block-uniform
    const int job = (int)(blockIdx.x / spj);
    const int64_t sb = (int64_t)blockIdx.x - (int64_t)job * spj;
    score_slots(jobs, segs, w, mu, sigma, slot_part, job, sb, slot_n,
                reinterpret_cast<double*>(s_stage), qP, qS);
    return;
  }
  const unsigned bid = (unsigned)((int64_t)blockIdx.x - slot_blocks);
  // one (job, tile) work item
  auto tile = [&](int job, int64_t base) __attribute__((always_inline)) {
    const tpe_job J = jobs[job];
    const int64_t n_lim = min(J.n_cand, limit);
    if (base >= n_lim || base < start) return;
    const tpe_seg SB = segs[J.below];
    const bool lgmm = J.family == TPE_LGMM1;
    const bool lo_on = J.flags & TPE_F_LOW, hi_on = J.flags & TPE_F_HIGH;
    // the first kLatLds slots of the lattice are deduplicated in LDS (for the
    // wide lattices of unbounded labels that is where the mass sits); slots
    // beyond go to the global marks directly, each read before its atomic
    const int n_loc = (int)min((int64_t)kLatLds, J.lat_n);
    for (int s = threadIdx.x; s < n_loc; s += kBS) lfirst[s] = 0xFFFFFFFFu;
    const Mix M = stage_mix(SB, wcdf, mu, sigma, s_mix);
    __syncthreads();
    if constexpr (POW2) {
      // kLatR consecutive candidates per thread (draw32_pairs); q a power of two:
      // x * (1/q) is exact in fp32, so rintf gives np.round(x / q) (tpe.py:106)
      // exactly and the slot needs no fp64 work
      const int64_t t0 = base + (int64_t)threadIdx.x * kLatR;
      const int nv = (int)max((int64_t)0, min((int64_t)kLatR, n_lim - t0));
      float x[kLatR];
      draw32_pairs<kLatR>(M, J.key, J.cand_base + t0, nv, lo_on, hi_on, bound32(J.low),
                          bound32(J.high), lgmm, s_stage + (threadIdx.x / kWave) * (kLatR * kWave), s_list + (threadIdx.x / kWave) * kRetryList,
                          x);
      const float inv_q32 = (float)(1.0 / J.q);
      const int kmin = (int)J.lat_kmin, nl = (int)J.lat_n;
#pragma unroll
      for (int r = 0; r < kLatR; ++r) {
        if (r >= nv) continue;
        const float t = rintf(x[r] * inv_q32);
        const int slot = (fabsf(t) < 2147483648.0f) ? (int)t - kmin : -1;
        if (slot < 0 || slot >= nl) {
          atomicOr(err, 2);
          continue;
        }
        // most draws land on slots already holding a smaller index: a plain read
        // first keeps the atomics (and their same-address serialisation) rare
        const uint32_t rel = (uint32_t)(t0 + r - base);
#ifdef TPE_DIAG_NO_MARK  // diagnostic builds only: slots computed, not marked
        if (rel == 0xFFFFFFFFu) lfirst[slot] = rel;
#else
        if (rel < lfirst[slot]) atomicMin(&lfirst[slot], rel);
#endif
      }
    } else {
      // np.round(x / q) (tpe.py:106) without a division per draw: t = x * (1/q) is
      // within 3.4e-16 |t| of fl(x / q), so rint(t) == rint(fl(x / q)) unless
      // fl(x / q) sits that close to a half-integer -- those few redo the division
      const double inv_q = 1.0 / J.q;
      auto mark = [&](double v, int64_t li) {
        const double t = v * inv_q;
        double k = rint(t);
        if (fabs(fabs(t - k) - 0.5) <= 8e-16 * fabs(t)) k = rint(v / J.q);
        const int64_t slot = (int64_t)k - J.lat_kmin;
        if (slot < 0 || slot >= J.lat_n) {
          atomicOr(err, 2);
          return;
        }
        if (slot < n_loc) {
          const uint32_t rel = (uint32_t)(li - base);
          if (rel < lfirst[slot]) atomicMin(&lfirst[slot], rel);
        } else {
          unsigned long long* dst = &slot_first[J.lat_off + slot];
          const unsigned long long g = (unsigned long long)(J.cand_base + li);
          if (g < __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(dst, g);
        }
      };
      if (J.flags & TPE_F_DRAW32) {
        const int64_t t0 = base + (int64_t)threadIdx.x * kLatR;
        const int nv = (int)max((int64_t)0, min((int64_t)kLatR, n_lim - t0));
        float x[kLatR];
        draw32_pairs<kLatR>(M, J.key, J.cand_base + t0, nv, lo_on, hi_on, bound32(J.low),
                            bound32(J.high), lgmm, s_stage + (threadIdx.x / kWave) * (kLatR * kWave), s_list + (threadIdx.x / kWave) * kRetryList,
                            x);
#pragma unroll
        for (int r = 0; r < kLatR; ++r)
          if (r < nv) mark((double)x[r], t0 + r);
      } else {
        for (int r = 0; r < kLatR; ++r) {
          const int64_t li = base + r * kBS + threadIdx.x;
          if (li >= n_lim) break;
          double v = draw64(M, J.key, J.cand_base + li, lo_on, hi_on, J.low, J.high);
          if (lgmm) v = exp(v);
          mark(v, li);
        }
      }
    }
    __syncthreads();
    // blocks run roughly in index order, so the global slot mostly holds a
    // smaller index already: an agent-scope load first keeps the (cross-XCD)
    // atomics to the blocks that improve a slot
#ifdef TPE_DIAG_NO_FLUSH  // diagnostic builds only: block results dropped
    if (n_loc > 0x7FFFFFF0)
#endif
    for (int s = threadIdx.x; s < n_loc; s += kBS) {
      const uint32_t f = lfirst[s];
      if (f == 0xFFFFFFFFu) continue;
      unsigned long long* dst = &slot_first[J.lat_off + s];
      const unsigned long long g = (unsigned long long)(J.cand_base + base + f);
      if (g < __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(dst, g);
    }
  };  // tile
  const int64_t tb = (int64_t)kBS * kLatR;
  if (!need) {
    // XCD-aware work order (as k_score_table): each XCD sweeps a contiguous
    // eighth of the (job, tile) list, so a job's first-index atomics stay in
    // few XCDs' L2s
    const int64_t W = (int64_t)n_tiles * n_jobs, per = (W + 7) / 8;
    const int64_t wi = (int64_t)(bid & 7) * per + (bid >> 3);
    if (wi >= W) return;
    const int job = (int)(wi / n_tiles);
    tile(job, (wi - (int64_t)job * n_tiles) * tb);
  } else {
    // the conditional rest of the streams: a grid-stride loop over the tiles
    // of the jobs whose flag is set, so a launch whose jobs are all settled is
    // a small grid that reads the flags and exits (a one-tile-per-block grid
    // of ~10^4 such blocks cost ~80 us of dispatch)
    for (int job = 0; job < n_jobs; ++job) {
      if (!need[job]) continue;  // block-uniform
      for (int64_t t = bid; t < n_tiles; t += (int64_t)gridDim.x - slot_blocks) {
        __syncthreads();  // the previous tile's LDS reads are done
        tile(job, t * tb);
      }
    }
  }
}

__global__ __launch_bounds__(kBS) void k_lattice_compact(
    const tpe_job* __restrict__ jobs, const unsigned long long* __restrict__ slot_first,
    double* __restrict__ vals, int64_t* __restrict__ firsts,
    unsigned long long* __restrict__ counts) {
  const tpe_job J = jobs[blockIdx.y];
  const int64_t s = (int64_t)blockIdx.x * kBS + threadIdx.x;
  if (s >= J.lat_n) return;
  const unsigned long long f = slot_first[J.lat_off + s];
  if (f == ~0ull) return;
  const unsigned long long pos = atomicAdd(&counts[blockIdx.y], 1ull);
  vals[J.lat_off + pos] = (double)(J.lat_kmin + s) * J.q;  // np.round(x/q) * q
  firsts[J.lat_off + pos] = (int64_t)f;
}

// Can the sampler put a draw on slot s at all?  Only unseen slots that could
// win ask; a "yes" costs the rest of the stream, a wrong "no" would cost
// parity, so the test is a superset: some below component's draw range
// (mean +- 5.8 sigma for fp32 Box-Muller draws, 8.7 for fp64 ones, widened
// for fp32 rounding) meets the slot's rounding bin, and the bin meets the
// bounds -- or holds a bound, where the sampler's last-resort clamp lands.
// (The lattice brackets the bounds with a slot on each side that no draw
// reaches; their probability mass is negative or 0/0, their score NaN.)
__device__ __forceinline__ bool slot_reachable(const tpe_job& J, const tpe_seg& SB,
                                               const double* __restrict__ mu,
                                               const double* __restrict__ sigma, int64_t s) {
  const double k = (double)(J.lat_kmin + s);
  double lo = (k - 0.5) * J.q, hi = (k + 0.5) * J.q;  // the bin of np.round(x / q) == k
  if (J.family == TPE_LGMM1) {  // the sampler's coordinate: log x
    if (!(hi > 0.0)) return false;
    lo = lo > 0.0 ? log(lo) : -INFINITY;
    hi = log(hi);
  }
  const double m = 1e-6 * (fabs(lo) + fabs(hi)) + 1e-300;
  lo -= m;
  hi += m;
  const bool lo_on = J.flags & TPE_F_LOW, hi_on = J.flags & TPE_F_HIGH;
  if (lo_on && hi < J.low) return false;
  if (hi_on && lo > J.high) return false;
  if ((lo_on && lo <= J.low && J.low <= hi) || (hi_on && lo <= J.high && J.high <= hi))
    return true;
  const double z = (J.flags & TPE_F_DRAW32) ? 5.8 : 8.7;
  for (int c = 0; c <= SB.n_obs; ++c) {
    const double mc = mu[SB.comp_off + c], r = z * sigma[SB.comp_off + c];
    const double mm = 1e-6 * (fabs(mc) + r);
    if (mc - r - mm <= hi && lo <= mc + r + mm) return true;
  }
  return false;
}

// one block per job; seen-ness and first indices from slot_first.  pass 0:
// best over the seen slots, need = an unseen, reachable slot could win (jobs
// whose whole stream was the prefix never need more); pass 1 (need jobs
// only): best over every slot seen in the whole stream
__global__ __launch_bounds__(kBS) void k_lattice_decide(
    const tpe_job* __restrict__ jobs, const tpe_seg* __restrict__ segs,
    const double* __restrict__ mu, const double* __restrict__ sigma,
    const tpe_best* __restrict__ partial, int64_t nper,
    const unsigned long long* __restrict__ slot_first, int64_t prefix, int pass,
    int32_t* __restrict__ need, tpe_best* __restrict__ best) {
  __shared__ BestT red[kBS / kWave];
  const int j = blockIdx.x;
  if (pass == 1 && !need[j]) return;  // block-uniform
  const tpe_job J = jobs[j];
  const tpe_best* P = partial + (int64_t)j * nper;
  const unsigned long long* F = slot_first + J.lat_off;
  BestT b{0.0, -1, 0.0};
  for (int64_t s = threadIdx.x; s < J.lat_n; s += kBS) {
    const unsigned long long f = F[s];
    if (f != ~0ull) best_update(b, P[s].score, (int64_t)f, P[s].value);
  }
  b = block_best<kBS>(b, red);
  int open = 0;
  if (pass == 0 && J.n_cand > prefix) {
    for (int64_t s = threadIdx.x; s < J.lat_n && !open; s += kBS)
      open = F[s] == ~0ull && better(P[s].score, INT64_MAX, b.score, b.index) &&
             slot_reachable(J, segs[J.below], mu, sigma, s);
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

// k_lattice_sample over candidates [start, min(n_cand, limit)) of every job
// (of the jobs with need[j] set, when need is given); false (error set) when
// the grid is too large
static bool launch_lattice_sample(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                                  const tpe_seg* segs, const double* mu, const double* sigma,
                                  const double* wcdf, uint64_t* slot_first, int32_t* err,
                                  int64_t start, int64_t limit, const int32_t* need,
                                  hipStream_t st, const char* who, const double* w = nullptr,
                                  tpe_best* slot_part = nullptr, int64_t slot_n = 0,
                                  const double* qP = nullptr, const double* qS = nullptr) {
  int64_t gx = 1;
  for (int i = 0; i < n_jobs; ++i) {
    const int64_t n = std::min(host_jobs[i].n_cand, limit);
    gx = std::max(gx, (n + (int64_t)kBS * kLatR - 1) / ((int64_t)kBS * kLatR));
  }
  const int64_t sblocks = need ? 0 : slot_n * n_jobs;  // slot scoring rides on the prefix launch
  const int64_t padded = xcd_grid(who, gx, n_jobs, sblocks);
  if (padded < 0) return false;
  bool pow2 = true;
  int64_t n_loc = 1;
  for (int i = 0; i < n_jobs; ++i) {
    pow2 = pow2 && lattice_pow2(host_jobs[i]);
    n_loc = std::max(n_loc, std::min((int64_t)kLatLds, host_jobs[i].lat_n));
  }
  const size_t lds = (size_t)n_loc * sizeof(uint32_t);
  unsigned long long* sf = (unsigned long long*)slot_first;
  // with need: a grid-stride grid (k_lattice_sample): two blocks per CU
  const unsigned grid = need ? (unsigned)std::min<int64_t>(padded, 512) : (unsigned)(padded + sblocks);
  const int sn = need ? 0 : (int)slot_n;  // (slot_n <= sblocks, which xcd_grid fitted to an int)
  dispatch_bool(pow2, [&](auto POW2) {
    hipLaunchKernelGGL(k_lattice_sample<decltype(POW2)::value>, dim3(grid), dim3(kBS), lds, st,
                       jobs, segs, mu, sigma, wcdf, sf, err, (int)gx, n_jobs, start, limit, need,
                       w, slot_part, sn, qP, qS);
  });
  return true;
}

extern "C" int tpe_lattice_sample(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                                  const tpe_seg* segs, const double* mu, const double* sigma,
                                  const double* wcdf, uint64_t* slot_first, int32_t* err,
                                  void* stream) {
  if (!check_jobs("tpe_lattice_sample", host_jobs, n_jobs)) return TPE_E_ARG;
  if (n_jobs == 0) return TPE_OK;
  if (!jobs || !segs || !mu || !sigma || !wcdf || !slot_first || !err) {
    set_error("tpe_lattice_sample: null pointer");
    return TPE_E_ARG;
  }
  int64_t end = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const tpe_job& j = host_jobs[i];
    if (!(j.flags & TPE_F_QUANT) || j.family == TPE_CAT || !(j.q > 0) || j.lat_n <= 0) {
      set_error("tpe_lattice_sample: job %d is not a quantized job with a lattice", i);
      return TPE_E_ARG;
    }
    end = std::max(end, j.lat_off + j.lat_n);
  }
  hipStream_t st = (hipStream_t)stream;
  bool ready = true;
  for (int i = 0; i < n_jobs; ++i) ready = ready && (host_jobs[i].flags & TPE_F_LATTICE_READY);
  if (!ready && hipMemsetAsync(slot_first, 0xFF, (size_t)end * sizeof(uint64_t), st) != hipSuccess)
    return check_launch("tpe_lattice_sample memset");
  if (!launch_lattice_sample(jobs, host_jobs, n_jobs, segs, mu, sigma, wcdf, slot_first, err, 0,
                             INT64_MAX, nullptr, st, "tpe_lattice_sample"))
    return TPE_E_UNSUPPORTED;
  return check_launch("tpe_lattice_sample");
}

extern "C" int tpe_lattice_suggest(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                                   const tpe_seg* segs, const double* w, const double* mu,
                                   const double* sigma, const double* wcdf, uint64_t* slot_first,
                                   int64_t prefix, tpe_best* partial, int64_t n_partial,
                                   int32_t* need, tpe_best* best, int32_t* err, double* reach_hi,
                                   double* reach_lo, void* stream) {
  if (!check_jobs("tpe_lattice_suggest", host_jobs, n_jobs)) return TPE_E_ARG;
  if (n_jobs == 0) return TPE_OK;
  if (!jobs || !segs || !w || !mu || !sigma || !wcdf || !slot_first || !partial || !need ||
      !best || !err) {
    set_error("tpe_lattice_suggest: null pointer");
    return TPE_E_ARG;
  }
  if (prefix <= 0 || prefix % ((int64_t)kBS * kLatR) != 0) {
    set_error("tpe_lattice_suggest: prefix %lld is not a positive multiple of %d",
              (long long)prefix, kBS * kLatR);
    return TPE_E_ARG;
  }
  int64_t end = 0, max_n = 1;
  for (int i = 0; i < n_jobs; ++i) {
    const tpe_job& j = host_jobs[i];
    if (!(j.flags & TPE_F_QUANT) || j.family == TPE_CAT || !(j.q > 0) || j.lat_n <= 0 ||
        (j.flags & TPE_F_INJECTED)) {
      set_error("tpe_lattice_suggest: job %d is not a sampled quantized job with a lattice", i);
      return TPE_E_ARG;
    }
    end = std::max(end, j.lat_off + j.lat_n);
    max_n = std::max(max_n, j.lat_n);
  }
  if (max_n > INT32_MAX || max_n * n_jobs > n_partial) {
    set_error("tpe_lattice_suggest: partial workspace %lld < %lld slots", (long long)n_partial,
              (long long)(max_n * n_jobs));
    return TPE_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  bool ready = true;
  for (int i = 0; i < n_jobs; ++i) ready = ready && (host_jobs[i].flags & TPE_F_LATTICE_READY);
  if (!ready && hipMemsetAsync(slot_first, 0xFF, (size_t)end * sizeof(uint64_t), st) != hipSuccess)
    return check_launch("tpe_lattice_suggest memset");
  unsigned long long* sf = (unsigned long long*)slot_first;
  const bool win = reach_hi && reach_lo;  // the slots' component windows (k_qreach)
  if (win)
    hipLaunchKernelGGL(k_qreach, dim3(4 * n_jobs), dim3(kQB), 0, st, jobs, segs, mu, sigma,
                       reach_hi, reach_lo);
  if (!launch_lattice_sample(jobs, host_jobs, n_jobs, segs, mu, sigma, wcdf, slot_first, err, 0,
                             prefix, nullptr, st, "tpe_lattice_suggest", w, partial, max_n,
                             win ? reach_hi : nullptr, win ? reach_lo : nullptr))
    return TPE_E_UNSUPPORTED;
  hipLaunchKernelGGL(k_lattice_decide, dim3(n_jobs), dim3(kBS), 0, st, jobs, segs, mu, sigma,
                     partial, max_n, sf, prefix, 0, need, best);
  bool more = false;
  for (int i = 0; i < n_jobs; ++i) more = more || host_jobs[i].n_cand > prefix;
  if (more) {  // the rest of the streams that need it (blocks of the others exit at once)
    if (!launch_lattice_sample(jobs, host_jobs, n_jobs, segs, mu, sigma, wcdf, slot_first, err,
                               prefix, INT64_MAX, need, st, "tpe_lattice_suggest"))
      return TPE_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_lattice_decide, dim3(n_jobs), dim3(kBS), 0, st, jobs, segs, mu, sigma,
                       partial, max_n, sf, prefix, 1, need, best);
  }
  return check_launch("tpe_lattice_suggest");
}

extern "C" int tpe_lattice_compact(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                                   const uint64_t* slot_first, double* vals, int64_t* firsts,
                                   int64_t* counts, void* stream) {
  if (!check_jobs("tpe_lattice_compact", host_jobs, n_jobs)) return TPE_E_ARG;
  if (n_jobs == 0) return TPE_OK;
  if (!jobs || !slot_first || !vals || !firsts || !counts) {
    set_error("tpe_lattice_compact: null pointer");
    return TPE_E_ARG;
  }
  int64_t maxn = 1;
  bool ready = true;
  for (int i = 0; i < n_jobs; ++i) {
    maxn = std::max(maxn, host_jobs[i].lat_n);
    ready = ready && (host_jobs[i].flags & TPE_F_LATTICE_READY);
  }
  hipStream_t st = (hipStream_t)stream;
  if (!ready && hipMemsetAsync(counts, 0, (size_t)n_jobs * sizeof(int64_t), st) != hipSuccess)
    return check_launch("tpe_lattice_compact memset");
  hipLaunchKernelGGL(k_lattice_compact, dim3((unsigned)((maxn + kBS - 1) / kBS), (unsigned)n_jobs),
                     dim3(kBS), 0, st, jobs, (const unsigned long long*)slot_first, vals, firsts,
                     (unsigned long long*)counts);
  return check_launch("tpe_lattice_compact");
}

extern "C" int64_t tpe_quantized_partials(const tpe_job* host_jobs, int n_jobs, int64_t max_vals) {
  (void)host_jobs;
  return (int64_t)n_jobs * std::max((int64_t)1, max_vals);  // one entry per value
}

extern "C" int tpe_score_quantized(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                                   const tpe_seg* segs, const double* w, const double* mu,
                                   const double* sigma, const double* vals,
                                   const int64_t* firsts, const int64_t* counts, int64_t max_vals,
                                   double* out_bl, double* out_al, tpe_best* partial,
                                   int64_t n_partial, tpe_best* best, int32_t* err,
                                   double* reach_hi, double* reach_lo, void* stream) {
  if (!check_jobs("tpe_score_quantized", host_jobs, n_jobs)) return TPE_E_ARG;
  if (n_jobs == 0) return TPE_OK;
  if (!jobs || !segs || !w || !mu || !sigma || !vals || !partial || !best || !err ||
      ((firsts == nullptr) != (counts == nullptr))) {
    set_error("tpe_score_quantized: null pointer (firsts and counts go together)");
    return TPE_E_ARG;
  }
  for (int i = 0; i < n_jobs; ++i)
    if (!(host_jobs[i].flags & TPE_F_QUANT) || !(host_jobs[i].q > 0) ||
        host_jobs[i].family == TPE_CAT) {
      set_error("tpe_score_quantized: job %d is not quantized", i);
      return TPE_E_ARG;
    }
  const int64_t gx = std::max((int64_t)1, max_vals);  // partial entries per job
  if (gx * n_jobs > n_partial) {
    set_error("tpe_score_quantized: partial workspace too small");
    return TPE_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const bool win = reach_hi && reach_lo;  // the values' component windows (k_qreach)
  if (win)
    hipLaunchKernelGGL(k_qreach, dim3(4 * n_jobs), dim3(kQB), 0, st, jobs, segs, mu, sigma,
                       reach_hi, reach_lo);
  hipLaunchKernelGGL(k_score_q, dim3((unsigned)gx, (unsigned)n_jobs),
                     dim3(kBS), 0, st, jobs, segs, w, mu, sigma, vals, firsts,
                     (const unsigned long long*)counts, out_bl, out_al, partial, err,
                     win ? reach_hi : nullptr, win ? reach_lo : nullptr, gx);
  launch_reduce(jobs, partial, gx, best, n_jobs, st);
  return check_launch("tpe_score_quantized");
}
