// tpe_joint_refine.hip -- the picked rows climb the joint criterion
// (tpe.suggest_sampled(joint=True, refine=N), tpe.refine_configs; the model:
// hyperopt_amd/joint.py "Refining").
//
// On the continuous labels J(t) = log L_below(t) - log L_above(t) is smooth in
// the fit coordinate t, with per set
//
//   r_i      = exp(a_i - log L)
//   dlogL_d  = sum_i r_i (mu_{i,d} - t_d) / sigma_{i,d}^2
//
// and a row moves by t' = clamp(t + h s^2 g), g = dlogL_below - dlogL_above, s
// the below set's bandwidths: with h = 1 and no above term the mean-shift step
// of the below mixture.  A step is kept when J rises (then h = min(1, 2 h)),
// else h halves; `refine` steps at the most, none once h < 2^-20.
//
// The shape is the reverse of the scorers': a handful of rows against 10^4
// components, refine + 1 evaluations in sequence.  So
//
//   one block per row, the whole climb in one launch;
//   components strided over the block's 256 threads: the prepared set's JComp
//     array is label-major D x C, a wave reads 64 consecutive components of a
//     label;
//   a thread walks its components once per evaluation and keeps an online
//     (m, s, w[D_c]) in registers -- the running maximum of a_i, the sum of
//     exp(a_i - m) and the D_c sums of exp(a_i - m) (mu - t) / sigma^2,
//     rescaled when m rises: value and gradient from one walk;
//   the pairs merge across the wave by a butterfly (four DPP steps inside a
//     row, two shuffles across rows; a merge is commutative bit for bit, so
//     every lane ends with the same bits), then across the four waves through
//     LDS in wave order;
//   LDS holds the row's t (current and trial), g, the moving labels' records
//     and the fixed labels' per-row inputs (a quantized label's clipped edges,
//     a discrete label's hit / miss / prior entries), formed once per row.
//     Their factors differ per component, so they stay in the walk; they are
//     added first, then the moving labels' in list order;
//   the block takes the accept / halve decision: every thread holds the same
//     J and h.
//
// The kernel is instantiated for D_c <= 4, 8 and 16 (the register arrays are
// indexed statically).  No atomics, every sum has a fixed order: a row's bits
// depend on the row, the two sets and `refine` only.
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

// one set's walk at the point t: every wave's (m, s, w) into out[wave]
template <int DC>
__device__ __forceinline__ void refine_walk(const double* __restrict__ set, int64_t n,
                                            int n_labels, const RShared<DC>& sh, int which,
                                            const double* t, double (*out)[2 + DC]) {
  const int64_t C = n + 1;
  const double* __restrict__ logw = set;
  const double* __restrict__ sig = set + C;
  const JComp* __restrict__ comp = reinterpret_cast<const JComp*>(set + set_comp_off(n_labels, C));
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

// J at the point t (every thread: the same bits), g into g_out[0, n_cont).
// Two block syncs: the waves' pairs are complete; g_out is.
template <int DC>
__device__ __forceinline__ double refine_eval(const double* __restrict__ set_b, int64_t n_b,
                                              const double* __restrict__ set_a, int64_t n_a,
                                              int n_labels, RShared<DC>& sh, const double* t,
                                              double* g_out) {
  refine_walk<DC>(set_b, n_b, n_labels, sh, 0, t, sh.red[0]);
  refine_walk<DC>(set_a, n_a, n_labels, sh, 1, t, sh.red[1]);
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

template <int DC>
__global__ __launch_bounds__(kJBS) void k_joint_refine(const tpe_joint_label* __restrict__ labels,
                                                       int n_labels,
                                                       const double* __restrict__ tables,
                                                       const double* __restrict__ set_b,
                                                       int64_t n_b,
                                                       const double* __restrict__ set_a,
                                                       int64_t n_a, double* __restrict__ vals,
                                                       int64_t ld, int refine,
                                                       double* __restrict__ J_start,
                                                       double* __restrict__ J_end,
                                                       double* __restrict__ g_end,
                                                       int32_t* __restrict__ accepted) {
  __shared__ RShared<DC> sh;
  const int64_t row = blockIdx.x;
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
    if (lab.kind == TPE_JOINT_QUANT) {  // (the edges of tpe_joint_pass.hpp's walk)
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
  double J = refine_eval<DC>(set_b, n_b, set_a, n_a, n_labels, sh, sh.t_cur, sh.g_cur);
  const double J0 = J;
  int acc = 0;
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
      const double Jn = refine_eval<DC>(set_b, n_b, set_a, n_a, n_labels, sh, sh.t_try, sh.g_try);
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
  if (tid < sh.n_cont) {
    const RCont& l = sh.cont[tid];
    const double t = sh.t_cur[tid];
    // a label that did not move keeps its stored bits (exp(log x) need not be x)
    if (t != sh.t0[tid]) vals[(int64_t)l.col * ld + row] = (l.flags & TPE_JOINT_LOG) ? exp(t) : t;
    if (g_end) g_end[row * sh.n_cont + tid] = sh.g_cur[tid];
  }
  if (tid == 0) {
    if (J_start) J_start[row] = J0;
    if (J_end) J_end[row] = J;
    if (accepted) accepted[row] = acc;
  }
}

template <int DC>
void launch_refine(int64_t n_rows, hipStream_t st, const tpe_joint_label* labels, int n_labels,
                   const double* tables, const double* set_b, int64_t n_b, const double* set_a,
                   int64_t n_a, double* vals, int64_t ld, int refine, double* J_start,
                   double* J_end, double* g_end, int32_t* accepted) {
  hipLaunchKernelGGL(k_joint_refine<DC>, dim3((unsigned)n_rows), dim3(kJBS), 0, st, labels,
                     n_labels, tables, set_b, n_b, set_a, n_a, vals, ld, refine, J_start, J_end,
                     g_end, accepted);
}
}  // namespace
}  // namespace tpe

using namespace tpe;

extern "C" int tpe_joint_refine(const tpe_joint_label* host_labels, const tpe_joint_label* labels,
                                int n_labels, const double* tables, int64_t n_tables,
                                const double* set_below, int64_t n_below, const double* set_above,
                                int64_t n_above, double* vals, int64_t ld, int n_cols,
                                int64_t n_rows, int refine, double* J_start, double* J_end,
                                double* g_end, int32_t* accepted, void* stream) {
  const int rc = check_joint_labels("tpe_joint_refine", host_labels, n_labels, n_cols,
                                    n_tables < 0 ? 0 : n_tables);
  if (rc != TPE_OK) return rc;
  if (n_below < 0 || n_above < 0 || n_below >= ((int64_t)1 << 40) ||
      n_above >= ((int64_t)1 << 40) || n_rows < 0 || ld < 0 || n_rows > ld ||
      n_rows > 2147483647 || refine < 0) {
    set_error("tpe_joint_refine: n=%lld / %lld, n_rows=%lld of ld=%lld, refine=%d",
              (long long)n_below, (long long)n_above, (long long)n_rows, (long long)ld, refine);
    return TPE_E_ARG;
  }
  bool cat = false;
  int n_cont = 0;
  for (int d = 0; d < n_labels; ++d) {
    cat |= host_labels[d].kind == TPE_JOINT_CAT;
    n_cont += host_labels[d].kind == TPE_JOINT_CONT;
  }
  if (n_cont > kRMaxCont) {
    set_error("tpe_joint_refine: %d continuous labels, at most %d", n_cont, kRMaxCont);
    return TPE_E_UNSUPPORTED;
  }
  // (no label moves: nothing to write unless the trace is wanted, and J once)
  if (n_rows == 0 || (n_cont == 0 && !J_start && !J_end && !accepted)) return TPE_OK;
  if (n_cont == 0) refine = 0;
  if (!labels || !set_below || !set_above || !vals || (cat && !tables)) {
    set_error("tpe_joint_refine: null pointer");
    return TPE_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  if (n_cont <= 4)
    launch_refine<4>(n_rows, st, labels, n_labels, tables, set_below, n_below, set_above, n_above,
                     vals, ld, refine, J_start, J_end, g_end, accepted);
  else if (n_cont <= 8)
    launch_refine<8>(n_rows, st, labels, n_labels, tables, set_below, n_below, set_above, n_above,
                     vals, ld, refine, J_start, J_end, g_end, accepted);
  else
    launch_refine<kRMaxCont>(n_rows, st, labels, n_labels, tables, set_below, n_below, set_above,
                             n_above, vals, ld, refine, J_start, J_end, g_end, accepted);
  return check_launch("tpe_joint_refine");
}

extern "C" int tpe_joint_refine_max_cont(void) { return kRMaxCont; }
