// tpe_joint_loo_label.hip -- the leave-one-out log-likelihood of a set's joint
// mixture as a function of ONE label's bandwidth multiplier, every other label
// held at its current one (tpe.joint_bandwidths, bandwidth="loo-label"; the
// model: hyperopt_amd/joint.py "Bandwidth per label").
//
// For a set of n rows, current multipliers h_e, label d and B grid values g_b:
// sigma_e = h_e sigma_p,e n^(-1/(D+4)) for e != d, sigma_d(b) = g_b sigma_p,d
// n^(-1/(D+4)), and a_ij, LOO_i, Q as tpe_joint_loo.hip states them.  The scalar
// walk folds every continuous label into one q_ij / s_b^2; here only label d
// moves with b, so a pair splits into what is fixed and what is d's:
//
//   rest_ij     -sum_{e != d} (u_i,e - u_j,e)^2 with u = t / (sqrt(2) sigma_e)
//               written pre-scaled by the prep (one subtract and one fma per
//               (pair, label), no scale to fetch), plus the discrete hit / miss
//               sum, plus one log_mass per quantized e != d at its fixed sigma:
//               once per pair, whatever B is.
//   d's own     continuous: q_d,ij = ((t_i - t_j) / (sqrt(2) sigma_p,d))^2 once
//               per pair and one fma with 1 / s_b^2 per b; quantized: one
//               log_mass per (pair, b).
//   j only      log v_j - sum_{e != d} (log(sigma_e sqrt(2 pi)) + log Z_e): n.
//   (j, b)      -log(sigma_d(b) sqrt(2 pi)) - log Z_d(mu_j, sigma_d(b)): B x n.
//
//   k_lool_prep   thread (j, b): b == 0 gathers the coordinates (label-major,
//                 D x n: u for a continuous label, t for a quantized one, the
//                 category of a discrete one), the quantized edges, the rest
//                 constant of j, and row j's prior component -- it depends on
//                 neither h nor b -- which it writes as the last "chunk" of
//                 every b's partials; every b writes label d's constant.
//   k_lool_pairs  grid row blocks x component chunks (kJBS, kJChunk); a thread
//                 owns row i and keeps B online (m, s) pairs in registers.  The
//                 chunk goes through LDS in passes of kJPer components: labels
//                 outside, rest_ij and q_d,ij of the pass in registers (the
//                 row's coordinates re-read per pass: D goes to 128); then per
//                 component (a rolled loop that rotates the two arrays) the B
//                 exponents join their (m, s), one exp each.  j == i and the
//                 places past n are reset to -inf before they can join.
//   k_lool_merge  per row and b: tpe_joint_pass.hpp's joint_merge over the chunks in
//                 chunk order and the prior's slot last, minus log(W - v_i),
//                 times v_i; a block tree over the rows.
//   k_loo_final   (tpe_joint_loo.hpp) thread b: the blocks in block order.
//
// k_lool_pairs is instantiated on B <= 4 / 8 / 16 and on (d quantized, another
// label quantized): a list without a quantized label never calls log_mass.  No
// atomics, every sum has a fixed order: out's bits depend on the inputs alone.
#include "tpe_joint_loo.hpp"
#include "tpe_joint_pass.hpp"

namespace tpe {
namespace {
// the labels' trial-component sigmas, by value to the prep (1 KiB of kernarg)
struct LabelSigma {
  double s[kJMaxD];
};

// the scratch, in doubles: partials (double2; per b: chunks + 1 slots of n) |
// coordinates | edges | rest constants | d's constants | sigma | block sums
struct LoolLayout {
  int64_t chunks, blocks, coord, edges, rest, cst, sig, blk, total;
};
inline LoolLayout lool_layout(int n_labels, int n_quant, int64_t n, int n_grid) {
  LoolLayout L;
  L.chunks = (n + kJChunk - 1) / kJChunk;
  L.blocks = (n + kJBS - 1) / kJBS;
  L.coord = 2 * (L.chunks + 1) * n_grid * n;
  L.edges = L.coord + (int64_t)n_labels * n;
  L.rest = L.edges + 2 * (int64_t)n_quant * n;
  L.cst = L.rest + n;
  L.sig = L.cst + (int64_t)n_grid * n;
  L.blk = L.sig + n_labels;
  L.total = L.blk + (int64_t)n_grid * L.blocks;
  return L;
}

__global__ __launch_bounds__(kJBS) void k_lool_prep(
    const tpe_joint_label* __restrict__ labels, int n_labels, const double* __restrict__ tables,
    const double* __restrict__ hvals, const uint8_t* __restrict__ hact, int64_t hld,
    const int32_t* __restrict__ rows, int64_t n, const double* __restrict__ wts, LabelSigma sg,
    int which, LooGrid g, int n_grid, double log_pw, int64_t n_chunks,
    double* __restrict__ coord, double* __restrict__ edges, double* __restrict__ rest,
    double* __restrict__ cst, double* __restrict__ sig, double2* __restrict__ partial) {
  const int64_t j = (int64_t)blockIdx.x * kJBS + threadIdx.x;
  const int b = blockIdx.y;
  if (j >= n) return;
  const int64_t row = rows ? (int64_t)rows[j] : j;
  const bool inside = row >= 0 && row < hld;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  {  // label d's constant under grid value b
    const tpe_joint_label lab = labels[which];
    const int64_t e = (int64_t)lab.col * hld + row;
    const double x = inside && hact[e] != 0 ? hvals[e] - lab.shift : nan;
    const double t = fit_coord(x, (lab.flags & TPE_JOINT_LOG) != 0);
    const double sigma = g.scale[b] * lab.prior_sigma;
    double c = (lab.flags & TPE_JOINT_BOUNDED) ? neg_log_z(lab, t, sigma) : 0.0;
    if (lab.kind == TPE_JOINT_CONT) c = c - log(sigma * sqrt(kTwoPi));
    cst[(int64_t)b * n + j] = c;
  }
  if (b != 0) return;
  if (j == 0)
    for (int d = 0; d < n_labels; ++d) sig[d] = sg.s[d];
  double acc = log(wts[j]), ap = log_pw;
  int qd = 0;
  for (int d = 0; d < n_labels; ++d) {
    const tpe_joint_label lab = labels[d];
    const bool is_log = (lab.flags & TPE_JOINT_LOG) != 0;
    const int64_t e = (int64_t)lab.col * hld + row;
    // (tpe_joint_prep's conversion of a history row)
    const double x = inside && hact[e] != 0 ? hvals[e] - lab.shift : nan;
    if (lab.kind == TPE_JOINT_CAT) {
      const int64_t cat = llrint(x);
      const bool in = cat >= 0 && cat < lab.n_cat;  // (a validated history: always)
      coord[(int64_t)d * n + j] = (double)cat;
      ap = ap + (in ? tables[lab.tab_off + 2 * (int64_t)lab.n_cat + cat] : kNegInf);
      continue;
    }
    const double t = fit_coord(x, is_log);
    const double sigma = sg.s[d];
    double prior = (lab.flags & TPE_JOINT_BOUNDED) ? neg_log_z(lab, lab.prior_mu, lab.prior_sigma)
                                                   : 0.0;
    if (lab.kind == TPE_JOINT_CONT) {
      // pre-scaled: by its own sigma where that is fixed, by sigma_p for label d
      coord[(int64_t)d * n + j] = t * (d == which ? lab.prior_r : 1.0 / (sqrt(2.0) * sigma));
      const double u = (t - lab.prior_mu) * lab.prior_r;
      prior = fma(-u, u, prior - log(lab.prior_sigma * sqrt(kTwoPi)));
      if (d != which) acc = acc - log(sigma * sqrt(kTwoPi));
    } else {  // (the edges of tpe_joint_pass.hpp's joint_walk)
      coord[(int64_t)d * n + j] = t;
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
      ++qd;
      prior = prior + log_mass(tu, tl, lab.prior_mu, lab.prior_sigma);
    }
    if (d != which && (lab.flags & TPE_JOINT_BOUNDED)) acc = acc + neg_log_z(lab, t, sigma);
    ap = ap + prior;
  }
  rest[j] = acc;
  // the prior component of row j: one more partial, after the last chunk
  for (int bb = 0; bb < n_grid; ++bb)
    partial[((int64_t)bb * (n_chunks + 1) + n_chunks) * n + j] = double2{ap, 1.0};
}

// DQ: label d is quantized (B masses per pair); OQ: some other label is (one each)
template <int NB, bool DQ, bool OQ>
__global__ __launch_bounds__(kJBS) void k_lool_pairs(
    const tpe_joint_label* __restrict__ labels, int n_labels, const double* __restrict__ tables,
    const double* __restrict__ coord, const double* __restrict__ edges,
    const double* __restrict__ rest, const double* __restrict__ cst,
    const double* __restrict__ sig, int64_t n, int which, int which_q, LooGrid g, int n_grid,
    int64_t n_chunks, double2* __restrict__ partial) {
  __shared__ double tile[kJMaxD * kJPer];     // the pass's coordinates, label-major
  __shared__ double ctile[(NB + 1) * kJPer];  // label d's constants, b-major; then the rest's
  __shared__ double qs[DQ ? NB * kJBS : 1];   // a component's masses of label d per (b, thread)
  const int tid = threadIdx.x;
  const int64_t chunk = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * kJBS + tid;
  const bool live = i < n;
  const int64_t ii = live ? i : 0;
  const int64_t j_first = chunk * kJChunk;
  const int64_t j_last = j_first + kJChunk < n ? j_first + kJChunk : n;
  const double xd = coord[(int64_t)which * n + ii];
  const double sigma_p = labels[which].prior_sigma;
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
      tile[e] = j0 + k < j_last ? coord[(int64_t)d * n + j0 + k] : 0.0;
    }
    for (int e = tid; e < (n_grid + 1) * kJPer; e += kJBS) {
      const int b = e / kJPer, k = e % kJPer;
      const double* __restrict__ src = b < n_grid ? cst + (int64_t)b * n : rest;
      ctile[(b < n_grid ? b : NB) * kJPer + k] = j0 + k < j_last ? src[j0 + k] : 0.0;
    }
    __syncthreads();
    // what does not depend on b: r = the rest constant - rest_ij, and q of label d
    double r[kJPer], q[kJPer];
#pragma unroll
    for (int k = 0; k < kJPer; ++k) {
      r[k] = ctile[NB * kJPer + k];
      q[k] = 0.0;
    }
    int qd = 0;
    for (int d = 0; d < n_labels; ++d) {
      const tpe_joint_label lab = labels[d];
      const double* __restrict__ t = tile + d * kJPer;
      if (d == which) {
        if (!DQ) {
#pragma unroll
          for (int k = 0; k < kJPer; ++k) {
            const double u = xd - t[k];
            q[k] = u * u;
          }
        }
        qd += DQ;
        continue;
      }
      const double x = coord[(int64_t)d * n + ii];
      if (lab.kind == TPE_JOINT_CONT) {
#pragma unroll
        for (int k = 0; k < kJPer; ++k) {
          const double u = x - t[k];
          r[k] = fma(-u, u, r[k]);
        }
      } else if (lab.kind == TPE_JOINT_CAT) {
        const int64_t cat = llrint(x);
        const bool in = cat >= 0 && cat < lab.n_cat;  // (a validated history: always)
        const double* __restrict__ tab = tables + lab.tab_off + (in ? cat : 0);
        const double hit = in ? tab[0] : kNegInf, miss = in ? tab[lab.n_cat] : kNegInf;
#pragma unroll
        for (int k = 0; k < kJPer; ++k) r[k] = r[k] + (t[k] == x ? hit : miss);
      } else if (OQ) {
        // two erf and a log per component: rolled, r[] rotates by one place per
        // step (every index static; back in place after kJPer steps)
        const double tu = edges[(int64_t)(2 * qd) * n + ii];
        const double tl = edges[(int64_t)(2 * qd + 1) * n + ii];
        const double sigma = sig[d];
        ++qd;
#pragma unroll 1
        for (int k = 0; k < kJPer; ++k) {
          // (a place past the chunk holds no component: no mass is formed for it)
          const double head = r[0] + (j0 + k < j_last ? log_mass(tu, tl, t[k], sigma) : 0.0);
#pragma unroll
          for (int p = 0; p + 1 < kJPer; ++p) r[p] = r[p + 1];
          r[kJPer - 1] = head;
        }
      }
    }
    // per component: a rolled loop (one set of exp bodies); r[] and q[] rotate
#pragma unroll 1
    for (int k = 0; k < kJPer; ++k) {
      const int64_t j = j0 + k;
      // itself, by index, and a place past the chunk: whatever the label loop
      // made of the zero pad, -inf takes its place before anything joins
      const bool out = j == i || j >= j_last;
      const double q0 = q[0], base = out ? kNegInf : r[0];
      if (DQ) {
        const double tu = edges[(int64_t)(2 * which_q) * n + ii];
        const double tl = edges[(int64_t)(2 * which_q + 1) * n + ii];
        const double mu = tile[which * kJPer + k];
        for (int b = 0; b < n_grid; ++b)  // (the thread's own slots: no sync)
          qs[b * kJBS + tid] = out ? 0.0 : log_mass(tu, tl, mu, g.scale[b] * sigma_p);
      }
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (b < n_grid) {
          double a = ctile[b * kJPer + k] + base;
          a = DQ ? a + qs[b * kJBS + tid] : fma(-q0, g.inv[b], a);
          loo_join(m[b], s[b], a);
        }
      }
#pragma unroll
      for (int p = 0; p + 1 < kJPer; ++p) {
        r[p] = r[p + 1];
        q[p] = q[p + 1];
      }
      r[kJPer - 1] = base;
      q[kJPer - 1] = q0;
    }
  }
  if (live) {
#pragma unroll
    for (int b = 0; b < NB; ++b)
      if (b < n_grid) partial[((int64_t)b * (n_chunks + 1) + chunk) * n + i] = double2{m[b], s[b]};
  }
}

// blk[b, block] = sum over the block's rows of v_i LOO_i(b)
__global__ __launch_bounds__(kJBS) void k_lool_merge(const double* __restrict__ wts, int64_t n,
                                                     const double2* __restrict__ all,
                                                     int64_t n_slots, int n_grid, double W,
                                                     double* __restrict__ blk) {
  __shared__ double red[kJBS];
  const int tid = threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x * kJBS + tid;
  const bool live = r < n;
  const double vi = live ? wts[r] : 0.0;
  const double log_rest = log(W - vi);
  for (int b = 0; b < n_grid; ++b) {
    double val = 0.0;
    if (live) {
      // (the slots: the chunks, then the prior's)
      const double v = joint_merge(all + (int64_t)b * n_slots * n, n_slots, n, r);
      val = vi * (v - log_rest);
    }
    __syncthreads();  // (the previous grid value's tree has been read)
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
void launch_lool_pairs(bool dq, bool oq, dim3 grid, hipStream_t st, const tpe_joint_label* labels,
                       int n_labels, const double* tables, const double* coord,
                       const double* edges, const double* rest, const double* cst,
                       const double* sig, int64_t n, int which, int which_q, const LooGrid& g,
                       int n_grid, int64_t n_chunks, double2* partial) {
#define TPE_LOOL_LAUNCH(DQ, OQ)                                                                 \
  hipLaunchKernelGGL((k_lool_pairs<NB, DQ, OQ>), grid, dim3(kJBS), 0, st, labels, n_labels,     \
                     tables, coord, edges, rest, cst, sig, n, which, which_q, g, n_grid,        \
                     n_chunks, partial)
  if (dq && oq)
    TPE_LOOL_LAUNCH(true, true);
  else if (dq)
    TPE_LOOL_LAUNCH(true, false);
  else if (oq)
    TPE_LOOL_LAUNCH(false, true);
  else
    TPE_LOOL_LAUNCH(false, false);
#undef TPE_LOOL_LAUNCH
}
}  // namespace
}  // namespace tpe

using namespace tpe;

extern "C" int64_t tpe_joint_loo_label_scratch_bytes(int n_labels, int n_quant, int64_t n,
                                                     int n_grid) {
  if (n_labels < 0 || n_labels > kJMaxD || n_quant < 0 || n_quant > n_labels || n < 0 ||
      n >= ((int64_t)1 << 40) || n_grid < 1 || n_grid > kLMaxB)
    return -1;
  return 8 * lool_layout(n_labels, n_quant, n, n_grid).total;
}

extern "C" int tpe_joint_loo_label(const tpe_joint_label* host_labels,
                                   const tpe_joint_label* labels, int n_labels,
                                   const double* tables, int64_t n_tables,
                                   const double* hist_vals, const uint8_t* hist_active,
                                   int64_t hist_ld, int hist_cols, const int32_t* rows, int64_t n,
                                   const double* v, double sum_v, double prior_weight,
                                   const double* mult, int which, const double* grid, int n_grid,
                                   double* out, void* scratch, void* stream) {
  const char* fn = "tpe_joint_loo_label";
  const int rc = check_joint_labels(fn, host_labels, n_labels, hist_cols,
                                    n_tables < 0 ? 0 : n_tables);
  if (rc != TPE_OK) return rc;
  if (n < 0 || hist_ld < 0 || (!rows && n > hist_ld) || n >= ((int64_t)1 << 40)) {
    set_error("%s: n=%lld hist_ld=%lld", fn, (long long)n, (long long)hist_ld);
    return TPE_E_ARG;
  }
  if (which < 0 || which >= n_labels || host_labels[which].kind == TPE_JOINT_CAT) {
    set_error("%s: which=%d: a continuous or quantized label of the %d", fn, which, n_labels);
    return TPE_E_ARG;
  }
  if (!grid || n_grid < 1 || n_grid > kLMaxB) {
    set_error("%s: n_grid=%d: 1 .. %d multipliers", fn, n_grid, kLMaxB);
    return TPE_E_ARG;
  }
  for (int b = 0; b < n_grid; ++b) {
    if (!(grid[b] > 0.0) || !(grid[b] < INFINITY) || (b && !(grid[b] > grid[b - 1]))) {
      set_error("%s: grid[%d]=%g: ascending, finite, > 0", fn, b, grid[b]);
      return TPE_E_ARG;
    }
  }
  if (!mult) {
    set_error("%s: null pointer", fn);
    return TPE_E_ARG;
  }
  bool cat = false;
  int n_quant = 0, which_q = 0;
  for (int d = 0; d < n_labels; ++d) {
    const int kind = host_labels[d].kind;
    cat |= kind == TPE_JOINT_CAT;
    if (kind == TPE_JOINT_QUANT && d < which) ++which_q;
    n_quant += kind == TPE_JOINT_QUANT;
    if (kind != TPE_JOINT_CAT && d != which && (!(mult[d] > 0.0) || !(mult[d] < INFINITY))) {
      set_error("%s: mult[%d]=%g: finite, > 0", fn, d, mult[d]);
      return TPE_E_ARG;
    }
  }
  if (!(prior_weight >= 0.0) || !(prior_weight < INFINITY)) {
    set_error("%s: prior_weight=%g", fn, prior_weight);
    return TPE_E_ARG;
  }
  if (!out) {
    set_error("%s: null pointer", fn);
    return TPE_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  if (n < 2) {  // nothing in the set depends on a bandwidth: Q = 0
    hipLaunchKernelGGL(k_loo_final, dim3(1), dim3(kWave), 0, st, (const double*)nullptr,
                       (int64_t)0, n_grid, 1.0, out);
    return check_launch(fn);
  }
  if (!labels || !hist_vals || !hist_active || !v || !scratch || (cat && !tables)) {
    set_error("%s: null pointer", fn);
    return TPE_E_ARG;
  }
  if (!(sum_v > 0.0) || !(sum_v < INFINITY)) {
    set_error("%s: sum_v=%g", fn, sum_v);
    return TPE_E_ARG;
  }
  const LoolLayout L = lool_layout(n_labels, n_quant, n, n_grid);
  if (L.blocks > 2147483647 || L.chunks > 65535) {
    set_error("%s: n=%lld does not fit a launch", fn, (long long)n);
    return TPE_E_ARG;
  }
  const double root = pow((double)n, -1.0 / (n_labels + 4));
  LooGrid g;
  for (int b = 0; b < kLMaxB; ++b) {
    g.scale[b] = (b < n_grid ? grid[b] : 1.0) * root;
    g.inv[b] = 1.0 / (g.scale[b] * g.scale[b]);
  }
  LabelSigma sg;
  for (int d = 0; d < kJMaxD; ++d) {
    const bool has = d < n_labels && d != which && host_labels[d].kind != TPE_JOINT_CAT;
    sg.s[d] = has ? mult[d] * root * host_labels[d].prior_sigma : 1.0;
  }
  double* base = static_cast<double*>(scratch);
  double2* partial = static_cast<double2*>(scratch);
  double *coord = base + L.coord, *edges = base + L.edges, *rest = base + L.rest;
  double *cst = base + L.cst, *sig = base + L.sig, *blk = base + L.blk;
  hipLaunchKernelGGL(k_lool_prep, dim3((unsigned)L.blocks, (unsigned)n_grid), dim3(kJBS), 0, st,
                     labels, n_labels, tables, hist_vals, hist_active, hist_ld, rows, n, v, sg,
                     which, g, n_grid, log(prior_weight), L.chunks, coord, edges, rest, cst, sig,
                     partial);
  const dim3 pairs((unsigned)L.blocks, (unsigned)L.chunks);
  const bool dq = host_labels[which].kind == TPE_JOINT_QUANT, oq = n_quant > (dq ? 1 : 0);
  if (n_grid <= 4)
    launch_lool_pairs<4>(dq, oq, pairs, st, labels, n_labels, tables, coord, edges, rest, cst,
                         sig, n, which, which_q, g, n_grid, L.chunks, partial);
  else if (n_grid <= 8)
    launch_lool_pairs<8>(dq, oq, pairs, st, labels, n_labels, tables, coord, edges, rest, cst,
                         sig, n, which, which_q, g, n_grid, L.chunks, partial);
  else
    launch_lool_pairs<kLMaxB>(dq, oq, pairs, st, labels, n_labels, tables, coord, edges, rest,
                              cst, sig, n, which, which_q, g, n_grid, L.chunks, partial);
  hipLaunchKernelGGL(k_lool_merge, dim3((unsigned)L.blocks), dim3(kJBS), 0, st, v, n,
                     (const double2*)partial, L.chunks + 1, n_grid, sum_v + prior_weight, blk);
  hipLaunchKernelGGL(k_loo_final, dim3(1), dim3(kWave), 0, st, (const double*)blk, L.blocks,
                     n_grid, sum_v, out);
  return check_launch(fn);
}
