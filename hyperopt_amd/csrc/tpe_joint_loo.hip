// tpe_joint_loo.hip -- the leave-one-out log-likelihood of a set's own joint
// mixture over a grid of bandwidth multipliers (tpe.joint_bandwidth,
// bandwidth="loo"; the model: hyperopt_amd/joint.py "Bandwidth").
//
// For a set of n rows, B multipliers h_b and sigma_d(h) = h sigma_p,d n^(-1/(D+4)):
//
//   a_ij(h)  = log v_j + sum_d log k_{d,j}(x_i,d; sigma(h))      j != i, by index
//   LOO_i(h) = logsumexp(a_i., a_i,prior) - log(W - v_i)
//   Q(h)     = sum_i v_i LOO_i(h) / sum_i v_i
//
// n^2 D B factor evaluations as written; a pair (i, j) is walked once for all B:
//
//   continuous   sum_d z^2 / 2 = q_ij / s_b^2, s_b = h_b n^(-1/(D+4)) and q_ij =
//                sum_d ((t_i,d - t_j,d) / (sqrt(2) sigma_p,d))^2 from the direct
//                differences: one fma per (pair, label), one per (pair, b).
//   discrete     the hit / miss sum does not depend on h: once per pair.
//   (j, b) only  log v_j - sum_d log(sigma_d sqrt(2 pi)) - sum_d log Z_d(mu_j,
//                sigma_d(h_b)): a B x n table, k_loo_prep.
//   quantized    log(Phi(ub) - Phi(lb)) per (pair, label, b), behind log_mass.
//
//   k_loo_prep   thread (j, b): gathers the fit coordinates mu (label-major,
//                D x n; the category of a discrete label), a quantized label's
//                clipped edges (b == 0), and the constant of (j, b).
//   k_loo_pairs  grid row blocks x component chunks (kJBS, kJChunk); a thread
//                owns row i and keeps B online (m, s) pairs in registers.  The
//                chunk goes through LDS in passes of kJPer components: labels
//                outside, the pass's q and hit / miss sums in registers; then per
//                component (a rolled loop that rotates the two arrays) the B
//                exponents join their (m, s), one exp each.  j == i and the
//                places past n are -inf.  Partials per (chunk, b, row).
//   k_loo_merge  per row and b: the chunks in chunk order, then the prior
//                component (it does not depend on b: once per row), minus
//                log(W - v_i), times v_i; a block tree over the rows.
//   k_loo_final  thread b: the block results in block order, over sum v.
//
// The (m, s) arrays are indexed statically: k_loo_pairs is instantiated for B <=
// 4, 8 and 16, and once more each for a label list with a quantized label (the
// calls of log_mass cost registers that a list without one does not pay).  No
// atomics, every sum has a fixed order: Q's bits depend on the inputs alone.
#include "tpe_joint_loo.hpp"

namespace tpe {
namespace {
// the scratch, in doubles: partials (double2) | mu | edges | constants | block sums
struct LooLayout {
  int64_t chunks, blocks, mu, edges, cst, blk, total;
};
inline LooLayout loo_layout(int n_labels, int n_quant, int64_t n, int n_grid) {
  LooLayout L;
  L.chunks = (n + kJChunk - 1) / kJChunk;
  L.blocks = (n + kJBS - 1) / kJBS;
  L.mu = 2 * L.chunks * n_grid * n;
  L.edges = L.mu + (int64_t)n_labels * n;
  L.cst = L.edges + 2 * (int64_t)n_quant * n;
  L.blk = L.cst + (int64_t)n_grid * n;
  L.total = L.blk + (int64_t)n_grid * L.blocks;
  return L;
}

// thread (j, b): component j's constant under multiplier b; b == 0 also gathers
__global__ __launch_bounds__(kJBS) void k_loo_prep(const tpe_joint_label* __restrict__ labels,
                                                   int n_labels,
                                                   const double* __restrict__ hvals,
                                                   const uint8_t* __restrict__ hact, int64_t hld,
                                                   const int32_t* __restrict__ rows, int64_t n,
                                                   const double* __restrict__ v, LooGrid g,
                                                   double* __restrict__ mu,
                                                   double* __restrict__ edges,
                                                   double* __restrict__ cst) {
  const int64_t j = (int64_t)blockIdx.x * kJBS + threadIdx.x;
  const int b = blockIdx.y;
  if (j >= n) return;
  const int64_t row = rows ? (int64_t)rows[j] : j;
  const double scale = g.scale[b];
  double acc = log(v[j]);
  int qd = 0;
  for (int d = 0; d < n_labels; ++d) {
    const tpe_joint_label lab = labels[d];
    const bool is_log = (lab.flags & TPE_JOINT_LOG) != 0;
    const int64_t e = (int64_t)lab.col * hld + row;
    const bool ok = row >= 0 && row < hld && hact[e] != 0;
    // (tpe_joint_prep's conversion of a history row)
    const double x = ok ? hvals[e] - lab.shift : __longlong_as_double(0x7FF8000000000000ll);
    const double t = lab.kind == TPE_JOINT_CAT ? (double)llrint(x) : fit_coord(x, is_log);
    if (b == 0) mu[(int64_t)d * n + j] = t;
    if (lab.kind == TPE_JOINT_QUANT) {
      if (b == 0) {  // (the edges of tpe_joint_pass.hpp's joint_walk)
        const double lb = x - 0.5 * lab.q;
        double tu = fit_coord(x + 0.5 * lab.q, is_log), tl = fit_coord(lb, is_log);
        if (lab.flags & TPE_JOINT_BOUNDED) {
          tu = fmin(fmax(tu, lab.lo), lab.hi);
          tl = fmin(fmax(tl, lab.lo), lab.hi);
        } else if (is_log && lb <= 0.0) {
          tl = kNegInf;  // normal_cdf(-inf) is exactly 0
        }
        edges[(int64_t)(2 * qd) * n + j] = tu;
        edges[(int64_t)(2 * qd + 1) * n + j] = tl;
      }
      ++qd;
    }
    if (lab.kind != TPE_JOINT_CAT) {
      const double sigma = scale * lab.prior_sigma;
      if (lab.flags & TPE_JOINT_BOUNDED) acc = acc + neg_log_z(lab, t, sigma);
      if (lab.kind == TPE_JOINT_CONT) acc = acc - log(sigma * sqrt(kTwoPi));
    }
  }
  cst[(int64_t)b * n + j] = acc;
}

template <int NB, bool QUANT>
__global__ __launch_bounds__(kJBS) void k_loo_pairs(const tpe_joint_label* __restrict__ labels,
                                                    int n_labels,
                                                    const double* __restrict__ tables,
                                                    const double* __restrict__ mu,
                                                    const double* __restrict__ edges,
                                                    const double* __restrict__ cst, int64_t n,
                                                    LooGrid g, int n_grid,
                                                    double2* __restrict__ partial) {
  __shared__ double tile[kJMaxD * kJPer];        // mu of the pass, label-major
  __shared__ double ctile[NB * kJPer];           // its constants, b-major
  __shared__ double qs[QUANT ? NB * kJBS : 1];   // a component's quantized sums per (b, thread)
  const int tid = threadIdx.x;
  const int64_t chunk = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * kJBS + tid;
  const bool live = i < n;
  const int64_t ii = live ? i : 0;
  const int64_t j_first = chunk * kJChunk;
  const int64_t j_last = j_first + kJChunk < n ? j_first + kJChunk : n;
  double m[NB], s[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    m[b] = kNegInf;
    s[b] = 0.0;
  }
  for (int64_t j0 = j_first; j0 < j_last; j0 += kJPer) {
    __syncthreads();  // (the previous pass has read the tiles)
    for (int e = tid; e < n_labels * kJPer; e += kJBS) {
      const int d = e / kJPer, k = e % kJPer;
      tile[e] = j0 + k < j_last ? mu[(int64_t)d * n + j0 + k] : 0.0;
    }
    for (int e = tid; e < n_grid * kJPer; e += kJBS) {
      const int b = e / kJPer, k = e % kJPer;
      ctile[e] = j0 + k < j_last ? cst[(int64_t)b * n + j0 + k] : 0.0;
    }
    __syncthreads();
    // what does not depend on h: q (continuous) and the hit / miss sum (discrete)
    double q[kJPer], c[kJPer];
#pragma unroll
    for (int k = 0; k < kJPer; ++k) q[k] = c[k] = 0.0;
    for (int d = 0; d < n_labels; ++d) {
      const tpe_joint_label lab = labels[d];
      const double x = mu[(int64_t)d * n + ii];
      const double* __restrict__ t = tile + d * kJPer;
      if (lab.kind == TPE_JOINT_CONT) {
        const double r = lab.prior_r;
#pragma unroll
        for (int k = 0; k < kJPer; ++k) {
          const double u = (x - t[k]) * r;
          q[k] = fma(u, u, q[k]);
        }
      } else if (lab.kind == TPE_JOINT_CAT) {
        const int64_t cat = llrint(x);
        const bool in = cat >= 0 && cat < lab.n_cat;  // (a validated history: always)
        const double* __restrict__ tab = tables + lab.tab_off + (in ? cat : 0);
        const double hit = in ? tab[0] : kNegInf, miss = in ? tab[lab.n_cat] : kNegInf;
#pragma unroll
        for (int k = 0; k < kJPer; ++k) c[k] = c[k] + (t[k] == x ? hit : miss);
      }
    }
    // per component: a rolled loop (one set of exp bodies); q[] and c[] rotate by
    // one place per step, so every index is static and after kJPer steps both
    // are back in place
#pragma unroll 1
    for (int k = 0; k < kJPer; ++k) {
      const int64_t j = j0 + k;
      const bool out = j == i || j >= j_last;  // itself, by index; a place past the chunk
      const double q0 = q[0], base = out ? kNegInf : c[0];
      if (QUANT) {
        // two erf and a log per (label, b): rolled, behind the non-inlined
        // log_mass (tpe_joint.hpp), the sums parked in LDS
        for (int b = 0; b < n_grid; ++b) {
          double sum = 0.0;
          if (!out) {
            int qd = 0;
            for (int d = 0; d < n_labels; ++d) {
              if (labels[d].kind != TPE_JOINT_QUANT) continue;
              const double tu = edges[(int64_t)(2 * qd) * n + ii];
              const double tl = edges[(int64_t)(2 * qd + 1) * n + ii];
              sum = sum + log_mass(tu, tl, tile[d * kJPer + k], g.scale[b] * labels[d].prior_sigma);
              ++qd;
            }
          }
          qs[b * kJBS + tid] = sum;  // (the thread's own slots: no sync)
        }
      }
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (b < n_grid) {
          double a = fma(-q0, g.inv[b], ctile[b * kJPer + k] + base);
          if (QUANT) a = a + qs[b * kJBS + tid];
          loo_join(m[b], s[b], a);
        }
      }
#pragma unroll
      for (int r = 0; r + 1 < kJPer; ++r) {
        q[r] = q[r + 1];
        c[r] = c[r + 1];
      }
      q[kJPer - 1] = q0;
      c[kJPer - 1] = base;
    }
  }
  if (live) {
#pragma unroll
    for (int b = 0; b < NB; ++b)
      if (b < n_grid) partial[(chunk * n_grid + b) * n + i] = double2{m[b], s[b]};
  }
}

// blk[b, block] = sum over the block's rows of v_i LOO_i(h_b)
__global__ __launch_bounds__(kJBS) void k_loo_merge(const tpe_joint_label* __restrict__ labels,
                                                    int n_labels,
                                                    const double* __restrict__ tables,
                                                    const double* __restrict__ mu,
                                                    const double* __restrict__ edges, int64_t n,
                                                    const double* __restrict__ v,
                                                    const double2* __restrict__ partial,
                                                    int64_t n_chunks, int n_grid, double log_pw,
                                                    double W, double* __restrict__ blk) {
  __shared__ double red[kJBS];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * kJBS + tid;
  const bool live = i < n;
  // the prior component of row i: the same under every multiplier
  double ap = log_pw, vi = 0.0;
  if (live) {
    vi = v[i];
    int qd = 0;
    for (int d = 0; d < n_labels; ++d) {
      const tpe_joint_label lab = labels[d];
      const double x = mu[(int64_t)d * n + i];
      if (lab.kind == TPE_JOINT_CAT) {
        const int64_t cat = llrint(x);
        const bool in = cat >= 0 && cat < lab.n_cat;
        ap = ap + (in ? tables[lab.tab_off + 2 * (int64_t)lab.n_cat + cat] : kNegInf);
        continue;
      }
      double term = (lab.flags & TPE_JOINT_BOUNDED) ? neg_log_z(lab, lab.prior_mu, lab.prior_sigma)
                                                    : 0.0;
      if (lab.kind == TPE_JOINT_CONT) {
        const double u = (x - lab.prior_mu) * lab.prior_r;
        term = fma(-u, u, term - log(lab.prior_sigma * sqrt(kTwoPi)));
      } else {
        term = term + log_mass(edges[(int64_t)(2 * qd) * n + i],
                               edges[(int64_t)(2 * qd + 1) * n + i], lab.prior_mu, lab.prior_sigma);
        ++qd;
      }
      ap = ap + term;
    }
  }
  const double log_rest = log(W - vi);
  for (int b = 0; b < n_grid; ++b) {
    double val = 0.0;
    if (live) {
      double m = ap;
      for (int64_t c = 0; c < n_chunks; ++c) {
        const double pm = partial[(c * n_grid + b) * n + i].x;
        m = pm > m ? pm : m;
      }
      double s = 0.0;
      for (int64_t c = 0; c < n_chunks; ++c) {  // (chunk order, the prior last)
        const double2 p = partial[(c * n_grid + b) * n + i];
        s = s + (p.x == kNegInf ? 0.0 : p.y * exp(p.x - m));
      }
      s = s + (ap == kNegInf ? 0.0 : exp(ap - m));
      const double loo = (m == kNegInf ? kNegInf : m + log(s)) - log_rest;
      val = vi * loo;
    }
    __syncthreads();  // (the previous multiplier's tree has been read)
    red[tid] = val;
    __syncthreads();
    for (int off = kJBS / 2; off > 0; off >>= 1) {
      if (tid < off) red[tid] = red[tid] + red[tid + off];
      __syncthreads();
    }
    if (tid == 0) blk[(int64_t)b * gridDim.x + blockIdx.x] = red[0];
  }
}

template <int NB>
void launch_pairs(bool quant, dim3 grid, hipStream_t st, const tpe_joint_label* labels,
                  int n_labels, const double* tables, const double* mu, const double* edges,
                  const double* cst, int64_t n, const LooGrid& g, int n_grid, double2* partial) {
  if (quant)
    hipLaunchKernelGGL((k_loo_pairs<NB, true>), grid, dim3(kJBS), 0, st, labels, n_labels, tables,
                       mu, edges, cst, n, g, n_grid, partial);
  else
    hipLaunchKernelGGL((k_loo_pairs<NB, false>), grid, dim3(kJBS), 0, st, labels, n_labels,
                       tables, mu, edges, cst, n, g, n_grid, partial);
}
}  // namespace
}  // namespace tpe

using namespace tpe;

extern "C" int tpe_joint_loo_max_grid(void) { return kLMaxB; }

extern "C" int64_t tpe_joint_loo_scratch_bytes(int n_labels, int n_quant, int64_t n,
                                               int n_grid) {
  if (n_labels < 0 || n_quant < 0 || n_quant > n_labels || n < 0 || n >= ((int64_t)1 << 40) ||
      n_grid < 1 || n_grid > kLMaxB)
    return -1;
  return 8 * loo_layout(n_labels, n_quant, n, n_grid).total;
}

extern "C" int tpe_joint_loo(const tpe_joint_label* host_labels, const tpe_joint_label* labels,
                             int n_labels, const double* tables, int64_t n_tables,
                             const double* hist_vals, const uint8_t* hist_active,
                             int64_t hist_ld, int hist_cols, const int32_t* rows, int64_t n,
                             const double* v, double sum_v, double prior_weight,
                             const double* grid, int n_grid, double* out, void* scratch,
                             void* stream) {
  const int rc = check_joint_labels("tpe_joint_loo", host_labels, n_labels, hist_cols,
                                    n_tables < 0 ? 0 : n_tables);
  if (rc != TPE_OK) return rc;
  if (n < 0 || hist_ld < 0 || (!rows && n > hist_ld) || n >= ((int64_t)1 << 40)) {
    set_error("tpe_joint_loo: n=%lld hist_ld=%lld", (long long)n, (long long)hist_ld);
    return TPE_E_ARG;
  }
  if (!grid || n_grid < 1 || n_grid > kLMaxB) {
    set_error("tpe_joint_loo: n_grid=%d: 1 .. %d multipliers", n_grid, kLMaxB);
    return TPE_E_ARG;
  }
  for (int b = 0; b < n_grid; ++b) {
    if (!(grid[b] > 0.0) || !(grid[b] < INFINITY) || (b && !(grid[b] > grid[b - 1]))) {
      set_error("tpe_joint_loo: grid[%d]=%g: ascending, finite, > 0", b, grid[b]);
      return TPE_E_ARG;
    }
  }
  if (!(prior_weight >= 0.0) || !(prior_weight < INFINITY)) {
    set_error("tpe_joint_loo: prior_weight=%g", prior_weight);
    return TPE_E_ARG;
  }
  if (!out) {
    set_error("tpe_joint_loo: null pointer");
    return TPE_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  if (n < 2) {  // nothing in the set depends on h: Q = 0
    hipLaunchKernelGGL(k_loo_final, dim3(1), dim3(kWave), 0, st, (const double*)nullptr,
                       (int64_t)0, n_grid, 1.0, out);
    return check_launch("tpe_joint_loo");
  }
  bool cat = false;
  int n_quant = 0;
  for (int d = 0; d < n_labels; ++d) {
    cat |= host_labels[d].kind == TPE_JOINT_CAT;
    n_quant += host_labels[d].kind == TPE_JOINT_QUANT;
  }
  if (!labels || !hist_vals || !hist_active || !v || !scratch || (cat && !tables)) {
    set_error("tpe_joint_loo: null pointer");
    return TPE_E_ARG;
  }
  if (!(sum_v > 0.0) || !(sum_v < INFINITY)) {
    set_error("tpe_joint_loo: sum_v=%g", sum_v);
    return TPE_E_ARG;
  }
  const LooLayout L = loo_layout(n_labels, n_quant, n, n_grid);
  if (L.blocks > 2147483647 || L.chunks > 65535) {
    set_error("tpe_joint_loo: n=%lld does not fit a launch", (long long)n);
    return TPE_E_ARG;
  }
  LooGrid g;
  const double root = pow((double)n, -1.0 / (n_labels + 4));
  for (int b = 0; b < kLMaxB; ++b) {
    g.scale[b] = (b < n_grid ? grid[b] : 1.0) * root;
    g.inv[b] = 1.0 / (g.scale[b] * g.scale[b]);
  }
  double* base = static_cast<double*>(scratch);
  double2* partial = static_cast<double2*>(scratch);
  double *mu = base + L.mu, *edges = base + L.edges, *cst = base + L.cst, *blk = base + L.blk;
  hipLaunchKernelGGL(k_loo_prep, dim3((unsigned)L.blocks, (unsigned)n_grid), dim3(kJBS), 0, st,
                     labels, n_labels, hist_vals, hist_active, hist_ld, rows, n, v, g, mu, edges,
                     cst);
  const dim3 pairs((unsigned)L.blocks, (unsigned)L.chunks);
  if (n_grid <= 4)
    launch_pairs<4>(n_quant > 0, pairs, st, labels, n_labels, tables, mu, edges, cst, n, g,
                    n_grid, partial);
  else if (n_grid <= 8)
    launch_pairs<8>(n_quant > 0, pairs, st, labels, n_labels, tables, mu, edges, cst, n, g,
                    n_grid, partial);
  else
    launch_pairs<kLMaxB>(n_quant > 0, pairs, st, labels, n_labels, tables, mu, edges, cst, n, g,
                         n_grid, partial);
  hipLaunchKernelGGL(k_loo_merge, dim3((unsigned)L.blocks), dim3(kJBS), 0, st, labels, n_labels,
                     tables, mu, edges, n, v, partial, L.chunks, n_grid, log(prior_weight),
                     sum_v + prior_weight, blk);
  hipLaunchKernelGGL(k_loo_final, dim3(1), dim3(kWave), 0, st, (const double*)blk, L.blocks,
                     n_grid, sum_v, out);
  return check_launch("tpe_joint_loo");
}
