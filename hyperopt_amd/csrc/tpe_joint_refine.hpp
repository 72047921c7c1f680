// tpe_joint_refine.hpp -- what the two climbs share (tpe_joint_refine.hip: the
// rows climb J over the always-live labels; tpe_joint_refine_tree.hip: every
// (row, live group) climbs its J_g): the per-row label records in LDS, the
// online (m, s, w[D_c]) walk of a set with its merges, J and g at a point, the
// accept / halve loop and the store of the labels that moved.
//
// A walk reads a set either from the prepared buffer or from a copy of it the
// block holds in LDS (RSet::stage_off; the tree kernel's staging).  Thread i
// owns components i, i + 256, ... in the same order in both, and the copy has
// the buffer's label-major layout: the source of a load differs, no operation
// does, so a staged and a streamed walk give the same bits.
#pragma once

#include "tpe_joint.hpp"

namespace tpe {
namespace {
constexpr int kRWaves = kJBS / kWave;
constexpr int kRMaxCont = TPE_REFINE_MAX_CONT;
constexpr double kRMinStep = 0x1.0p-20;

struct RFixed {  // a label that stays: its row of the component array and the row's inputs
  int32_t kind, d;
  // QUANT: the edges tu, tl in the fit coordinate; CAT: the category, then its
  // hit / miss / prior entries
  double p0, p1, p2, p3;
  double prior_sigma;
};

struct RCont {  // a label that moves
  int32_t d, flags, col, pad_;
  double lo, hi;
  double rp;      // 1 / (sqrt(2) sigma_p)
  double rt[2];   // 1 / (sqrt(2) sigma) of the trial components: below, above
  double step;    // s^2
};

template <int DC>
struct RShared {
  RFixed fixed[kJMaxD];
  RCont cont[DC];
  double t0[DC], t_cur[DC], t_try[DC], g_cur[DC], g_try[DC];
  double red[2][kRWaves][2 + DC];  // per set and wave: m, s, w[]
  int n_fixed, n_cont;
};

struct RSet {  // a prepared set of n + 1 components as a walk reads it
  const double* logw;
  const double* sig;
  const JComp* comp;
  int64_t n;
  int stage_off;  // where its copy starts in the block's stage, in doubles; -1: none
};

__device__ __forceinline__ RSet refine_set(const double* set, int64_t n, int n_labels) {
  const int64_t C = n + 1;
  return RSet{set, set + C, reinterpret_cast<const JComp*>(set + set_comp_off(n_labels, C)), n,
              -1};
}

// a staged set: log w (C, padded to an even count), then the JComp rows (D x C)
__host__ __device__ constexpr int64_t stage_comp_off(int64_t C) { return (C + 1) & ~(int64_t)1; }

// (m, s, w) <- (m, s, w) merged with (om, os, ow); commutative bit for bit
template <int DC>
__device__ __forceinline__ void refine_merge(double& m, double& s, double (&w)[DC], double om,
                                             double os, const double (&ow)[DC]) {
  const double M = om > m ? om : m;
  const double fa = m == kNegInf ? 0.0 : exp(m - M);
  const double fb = om == kNegInf ? 0.0 : exp(om - M);
  s = s * fa + os * fb;
#pragma unroll
  for (int j = 0; j < DC; ++j) w[j] = w[j] * fa + ow[j] * fb;
  m = M;
}

template <int CTRL, int DC>
__device__ __forceinline__ void refine_step_dpp(double& m, double& s, double (&w)[DC]) {
  double ow[DC];
  const double om = dpp_d<CTRL>(m), os = dpp_d<CTRL>(s);
#pragma unroll
  for (int j = 0; j < DC; ++j) ow[j] = dpp_d<CTRL>(w[j]);
  refine_merge<DC>(m, s, w, om, os, ow);
}

template <int DC>
__device__ __forceinline__ void refine_step_xor(double& m, double& s, double (&w)[DC], int off) {
  double ow[DC];
  const double om = __shfl_xor(m, off, kWave), os = __shfl_xor(s, off, kWave);
#pragma unroll
  for (int j = 0; j < DC; ++j) ow[j] = __shfl_xor(w[j], off, kWave);
  refine_merge<DC>(m, s, w, om, os, ow);
}

// one set's walk at the point t: every wave's (m, s, w) into out[wave].  logw
// and comp: the prepared buffer's, or their staged copies
template <int DC>
__device__ __forceinline__ void refine_walk(const double* __restrict__ logw,
                                            const double* __restrict__ sig,
                                            const JComp* __restrict__ comp, int64_t n,
                                            const RShared<DC>& sh, int which, const double* t,
                                            double (*out)[2 + DC]) {
  const int64_t C = n + 1;
  const int nf = sh.n_fixed, nc = sh.n_cont;
  double m = kNegInf, s = 0.0, w[DC];
#pragma unroll
  for (int j = 0; j < DC; ++j) w[j] = 0.0;
  for (int64_t i = threadIdx.x; i < C; i += kJBS) {
    const bool prior = i == n;
    double a = logw[i];
    for (int f = 0; f < nf; ++f) {
      const RFixed& x = sh.fixed[f];
      const JComp c = comp[(int64_t)x.d * C + i];
      if (x.kind == TPE_JOINT_QUANT)
        a = a + (log_mass(x.p0, x.p1, c.mu, prior ? x.prior_sigma : sig[x.d]) + c.cst);
      else
        a = a + (prior ? x.p3 : (c.mu == x.p0 ? x.p1 : x.p2));
    }
    double dl[DC];  // (mu - t) / sigma^2
#pragma unroll
    for (int j = 0; j < DC; ++j) {
      dl[j] = 0.0;
      if (j < nc) {
        const RCont& l = sh.cont[j];
        const JComp c = comp[(int64_t)l.d * C + i];
        const double r = prior ? l.rp : l.rt[which];
        const double diff = t[j] - c.mu, u = diff * r;
        a = a + fma(-u, u, c.cst);
        dl[j] = -diff * (2.0 * r * r);
      }
    }
    if (a > m) {  // (m = -inf: s and w are 0 and stay 0)
      const double sc = exp(m - a);
      s = s * sc;
#pragma unroll
      for (int j = 0; j < DC; ++j) w[j] = w[j] * sc;
      m = a;
    }
    if (a != kNegInf) {  // (a NaN makes s NaN: log L is NaN, as the scorer's)
      const double e = exp(a - m);
      s = s + e;
#pragma unroll
      for (int j = 0; j < DC; ++j) w[j] = fma(e, dl[j], w[j]);
    }
  }
  refine_step_dpp<kDppXor1, DC>(m, s, w);
  refine_step_dpp<kDppXor2, DC>(m, s, w);
  refine_step_dpp<kDppHalfMirror, DC>(m, s, w);
  refine_step_dpp<kDppMirror, DC>(m, s, w);
  refine_step_xor<DC>(m, s, w, 16);
  refine_step_xor<DC>(m, s, w, 32);
  if (lane_id() == 0) {
    double* o = out[threadIdx.x / kWave];
    o[0] = m;
    o[1] = s;
#pragma unroll
    for (int j = 0; j < DC; ++j) o[2 + j] = w[j];
  }
}

// the walk of the set `set` from where it lies: STAGED kernels hold `stage`, a
// block's LDS copy of the sets whose stage_off is not -1 (block-uniform)
template <int DC, bool STAGED>
__device__ __forceinline__ void refine_walk_set(const RSet& set, const double* stage,
                                                const RShared<DC>& sh, int which, const double* t,
                                                double (*out)[2 + DC]) {
  if (STAGED && set.stage_off >= 0) {
    const double* lw = stage + set.stage_off;
    refine_walk<DC>(lw, set.sig, reinterpret_cast<const JComp*>(lw + stage_comp_off(set.n + 1)),
                    set.n, sh, which, t, out);
  } else {
    refine_walk<DC>(set.logw, set.sig, set.comp, set.n, sh, which, t, out);
  }
}

// J at the point t (every thread: the same bits), g into g_out[0, n_cont).
// Two block syncs: the waves' pairs are complete; g_out is.
template <int DC, bool STAGED>
__device__ __forceinline__ double refine_eval(const RSet& set_b, const RSet& set_a,
                                              const double* stage, RShared<DC>& sh,
                                              const double* t, double* g_out) {
  refine_walk_set<DC, STAGED>(set_b, stage, sh, 0, t, sh.red[0]);
  refine_walk_set<DC, STAGED>(set_a, stage, sh, 1, t, sh.red[1]);
  __syncthreads();
  double L[2], M[2], S[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    double mx = kNegInf;
#pragma unroll
    for (int v = 0; v < kRWaves; ++v) mx = sh.red[q][v][0] > mx ? sh.red[q][v][0] : mx;
    double sum = 0.0;
#pragma unroll
    for (int v = 0; v < kRWaves; ++v) {
      const double mv = sh.red[q][v][0];
      sum = sum + (mv == kNegInf ? 0.0 : sh.red[q][v][1] * exp(mv - mx));
    }
    M[q] = mx;
    S[q] = sum;
    L[q] = mx == kNegInf ? kNegInf : mx + log(sum);
  }
  if ((int)threadIdx.x < sh.n_cont) {
    const int j = threadIdx.x;
    double g = 0.0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      double sum = 0.0;
#pragma unroll
      for (int v = 0; v < kRWaves; ++v) {
        const double mv = sh.red[q][v][0];
        sum = sum + (mv == kNegInf ? 0.0 : sh.red[q][v][2 + j] * exp(mv - M[q]));
      }
      const double dlog = M[q] == kNegInf ? 0.0 : sum / S[q];  // (an empty mixture: no pull)
      g = q == 0 ? dlog : g - dlog;
    }
    g_out[j] = g;
  }
  __syncthreads();
  return L[0] - L[1];
}

// the row's records: the two label lists in list order, the fixed labels'
// per-row inputs, the moving labels' records and the start point.  `labels`,
// `tables` and the two set buffers are one mixture pair's (a group's, with
// tab_off counted from `tables`); ends with a block sync
template <int DC>
__device__ __forceinline__ void refine_setup(const tpe_joint_label* __restrict__ labels,
                                             int n_labels, const double* __restrict__ tables,
                                             const double* __restrict__ set_b, int64_t n_b,
                                             const double* __restrict__ set_a, int64_t n_a,
                                             const double* vals, int64_t ld, int64_t row,
                                             RShared<DC>& sh) {
  const int tid = threadIdx.x;
  if (tid == 0) {  // the two label lists, in list order
    int nf = 0, nc = 0;
    for (int d = 0; d < n_labels; ++d) {
      if (labels[d].kind == TPE_JOINT_CONT) {
        if (nc < DC) sh.cont[nc++].d = d;  // (the entry point checked D_c <= DC)
      } else {
        sh.fixed[nf++].d = d;
      }
    }
    sh.n_fixed = nf;
    sh.n_cont = nc;
  }
  __syncthreads();
  for (int f = tid; f < sh.n_fixed; f += kJBS) {
    RFixed& x = sh.fixed[f];
    const tpe_joint_label lab = labels[x.d];
    const double v = vals[(int64_t)lab.col * ld + row];
    x.kind = lab.kind;
    x.prior_sigma = lab.prior_sigma;
    if (lab.kind == TPE_JOINT_QUANT) {  // (the edges of tpe_joint_pass.hpp's joint_walk)
      const bool is_log = (lab.flags & TPE_JOINT_LOG) != 0;
      const double lb = v - 0.5 * lab.q;
      double tu = fit_coord(v + 0.5 * lab.q, is_log), tl = fit_coord(lb, is_log);
      if (lab.flags & TPE_JOINT_BOUNDED) {
        tu = fmin(fmax(tu, lab.lo), lab.hi);
        tl = fmin(fmax(tl, lab.lo), lab.hi);
      } else if (is_log && lb <= 0.0) {
        tl = kNegInf;  // normal_cdf(-inf) is exactly 0
      }
      x.p0 = tu;
      x.p1 = tl;
      x.p2 = x.p3 = 0.0;
    } else {
      const int64_t c = llrint(v);
      const bool in = c >= 0 && c < lab.n_cat;  // (a validated pool: always)
      const double* __restrict__ tab = tables + lab.tab_off + (in ? c : 0);
      x.p0 = (double)c;
      x.p1 = in ? tab[0] : kNegInf;
      x.p2 = in ? tab[lab.n_cat] : kNegInf;
      x.p3 = in ? tab[2 * (int64_t)lab.n_cat] : kNegInf;
    }
  }
  if (tid < sh.n_cont) {
    RCont& l = sh.cont[tid];
    const tpe_joint_label lab = labels[l.d];
    l.flags = lab.flags;
    l.col = lab.col;
    l.lo = lab.lo;
    l.hi = lab.hi;
    l.rp = lab.prior_r;
    l.rt[0] = set_b[n_b + 1 + n_labels + l.d];
    l.rt[1] = set_a[n_a + 1 + n_labels + l.d];
    const double sd = n_b > 0 ? set_b[n_b + 1 + l.d] : lab.prior_sigma;
    l.step = sd * sd;
    const double t =
        fit_coord(vals[(int64_t)lab.col * ld + row], (lab.flags & TPE_JOINT_LOG) != 0);
    sh.t0[tid] = t;
    sh.t_cur[tid] = t;
  }
  __syncthreads();
}

// the climb from sh.t_cur: J at the point it ends on (sh.t_cur, sh.g_cur), the
// first J into J0, the steps kept into acc
template <int DC, bool STAGED>
__device__ __forceinline__ double refine_climb(const RSet& set_b, const RSet& set_a,
                                               const double* stage, RShared<DC>& sh, int refine,
                                               double& J0, int& acc) {
  const int tid = threadIdx.x;
  double J = refine_eval<DC, STAGED>(set_b, set_a, stage, sh, sh.t_cur, sh.g_cur);
  J0 = J;
  acc = 0;
  double h = 1.0;
  // (J, h and acc are the same in every thread: the loop is block-uniform)
  if (fabs(J) < INFINITY) {
    for (int it = 0; it < refine && h >= kRMinStep; ++it) {
      if (tid < sh.n_cont) {
        const RCont& l = sh.cont[tid];
        double t = sh.t_cur[tid] + (h * l.step) * sh.g_cur[tid];
        if (l.flags & TPE_JOINT_BOUNDED) {  // (draw64's clamp)
          if (t < l.lo) t = l.lo;
          if (!(t < l.hi)) t = nextafter(l.hi, -INFINITY);
        }
        sh.t_try[tid] = t;
      }
      __syncthreads();
      const double Jn = refine_eval<DC, STAGED>(set_b, set_a, stage, sh, sh.t_try, sh.g_try);
      if (Jn > J) {
        // (thread j alone reads and writes entry j of t_cur / g_cur from here on)
        if (tid < sh.n_cont) {
          sh.t_cur[tid] = sh.t_try[tid];
          sh.g_cur[tid] = sh.g_try[tid];
        }
        J = Jn;
        ++acc;
        h = fmin(1.0, 2.0 * h);
      } else {
        h = 0.5 * h;
      }
    }
  }
  return J;
}

// the moving labels' values back into the row, and g into g_row where it is wanted
template <int DC>
__device__ __forceinline__ void refine_store(const RShared<DC>& sh, double* vals, int64_t ld,
                                             int64_t row, double* g_row) {
  const int tid = threadIdx.x;
  if (tid < sh.n_cont) {
    const RCont& l = sh.cont[tid];
    const double t = sh.t_cur[tid];
    // a label that did not move keeps its stored bits (exp(log x) need not be x)
    if (t != sh.t0[tid]) vals[(int64_t)l.col * ld + row] = (l.flags & TPE_JOINT_LOG) ? exp(t) : t;
    if (g_row) g_row[tid] = sh.g_cur[tid];
  }
}
}  // namespace
}  // namespace tpe
