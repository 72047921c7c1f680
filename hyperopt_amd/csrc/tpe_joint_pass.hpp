// tpe_joint_pass.hpp -- the arithmetic of the joint criterion's scorers
// (k_joint_rows / k_joint_rows_merge in tpe_joint.hip; the merge also in
// tpe_grid_joint.hip and tpe_joint_loo_label.hip): a thread's walk over one
// chunk of components, and a row's merge of its chunks.  Every sum has a fixed
// order, so a row's bits depend on the row, the set and kJChunk / kJPer only.
#pragma once

#include "tpe_joint.hpp"

namespace tpe {
namespace {

// a pass's a[] joins a running (m, s), in component order.  a[] comes back as
// it was: the rolled loop (one exp body) rotates it by one place per step, so
// every index is static and the array stays in registers.
__device__ __forceinline__ void joint_join(double (&a)[kJPer], double& m, double& s) {
  double pm = a[0];
#pragma unroll
  for (int k = 1; k < kJPer; ++k) pm = a[k] > pm ? a[k] : pm;
  if (pm > m) {
    s = s * exp(m - pm);  // (m = -inf: s is 0 and stays 0)
    m = pm;
  }
#pragma unroll 1
  for (int k = 0; k < kJPer; ++k) {
    const double head = a[0];
    s = s + (head == kNegInf ? 0.0 : exp(head - m));
#pragma unroll
    for (int j = 0; j + 1 < kJPer; ++j) a[j] = a[j + 1];
    a[kJPer - 1] = head;
  }
}

// a place past the last component holds no component: whatever the label loop
// added to its -inf from the zero pad (a NaN where a factor was inf * 0), it
// counts for nothing
__device__ __forceinline__ void joint_clear_past(double (&a)[kJPer], int64_t i0, int64_t C) {
#pragma unroll
  for (int k = 0; k < kJPer; ++k)
    if (i0 + k >= C) a[k] = kNegInf;
}

struct JWalk {  // the running maximum and sum of a chunk's a_i; with a context,
  double m, s;  // the same pair over the a_i cut off after the first n_ctx labels
  double m_ctx, s_ctx;
};

// A thread's walk over the chunk of components that starts at i_first, for
// pool row `row`: passes of kJPer components whose a_i it keeps in registers,
// labels outside, components inside, the pass's {mu, constant} pairs staged in
// `tile` (kJMaxD * kJPer JComp of LDS) and read as broadcasts.  Every thread of
// the kJBS block walks it (it syncs on `tile`).  set: a prepared set of n
// trials.  kCtx: n_ctx in (0, n_labels); at the label boundary a[] holds the
// a_i of the first n_ctx labels, which join (m_ctx, s_ctx), and the walk goes
// on to the full a_i in the same registers.
template <bool kCtx>
__device__ __forceinline__ JWalk joint_walk(const tpe_joint_label* __restrict__ labels,
                                            int n_labels, int n_ctx,
                                            const double* __restrict__ tables,
                                            const double* __restrict__ set, int64_t n,
                                            const double* __restrict__ vals, int64_t ld,
                                            int64_t row, int64_t i_first, JComp* tile) {
  const int64_t C = n + 1;
  const double* __restrict__ logw = set;
  const double* __restrict__ sig = set + C;
  const JComp* __restrict__ comp = reinterpret_cast<const JComp*>(set + set_comp_off(n_labels, C));
  JWalk w{kNegInf, 0.0, kNegInf, 0.0};
  for (int64_t i0 = i_first; i0 < i_first + kJChunk && i0 < C; i0 += kJPer) {
    __syncthreads();  // (the previous pass has read the tile)
    for (int e = threadIdx.x; e < n_labels * kJPer; e += kJBS) {
      const int d = e / kJPer, k = e % kJPer;
      tile[e] = i0 + k < C ? comp[(int64_t)d * C + i0 + k] : JComp{0.0, 0.0};
    }
    __syncthreads();
    double a[kJPer];
#pragma unroll
    for (int k = 0; k < kJPer; ++k) a[k] = i0 + k < C ? logw[i0 + k] : kNegInf;
    const int k_prior = n - i0 < kJPer ? (int)(n - i0) : -1;  // the prior's place in this pass
    for (int d = 0; d < n_labels; ++d) {
      if constexpr (kCtx) {
        if (d == n_ctx) {
          joint_clear_past(a, i0, C);
          joint_join(a, w.m_ctx, w.s_ctx);
        }
      }
      const tpe_joint_label lab = labels[d];
      const double x = vals[(int64_t)lab.col * ld + row];
      const JComp* __restrict__ t = tile + d * kJPer;
      if (lab.kind == TPE_JOINT_CONT) {
        const double tx = fit_coord(x, (lab.flags & TPE_JOINT_LOG) != 0);
        const double rt = sig[n_labels + d], rp = lab.prior_r;
#pragma unroll
        for (int k = 0; k < kJPer; ++k) {
          const double u = (tx - t[k].mu) * (k == k_prior ? rp : rt);
          a[k] = a[k] + fma(-u, u, t[k].cst);
        }
      } else if (lab.kind == TPE_JOINT_QUANT) {
        const bool is_log = (lab.flags & TPE_JOINT_LOG) != 0;
        const bool bounded = (lab.flags & TPE_JOINT_BOUNDED) != 0;
        const double lb = x - 0.5 * lab.q;
        double tu = fit_coord(x + 0.5 * lab.q, is_log), tl = fit_coord(lb, is_log);
        if (bounded) {
          tu = fmin(fmax(tu, lab.lo), lab.hi);
          tl = fmin(fmax(tl, lab.lo), lab.hi);
        } else if (is_log && lb <= 0.0) {
          tl = kNegInf;  // normal_cdf(-inf) is exactly 0
        }
        const double sigma = sig[d];
        // two erf and a log per component: a rolled loop (unrolled, the 32
        // erf bodies took the kernel to 188 VGPRs).  a[] stays in registers
        // because the loop rotates it by one place per step: every index is
        // static, and after kJPer steps the array is back in place.
#pragma unroll 1
        for (int k = 0; k < kJPer; ++k) {
          const double sg = k == k_prior ? lab.prior_sigma : sigma;
          const double head = a[0] + (log_mass(tu, tl, t[k].mu, sg) + t[k].cst);
#pragma unroll
          for (int j = 0; j + 1 < kJPer; ++j) a[j] = a[j + 1];
          a[kJPer - 1] = head;
        }
      } else {
        const int64_t c = llrint(x);
        const bool in = c >= 0 && c < lab.n_cat;  // (a validated pool: always)
        const double* __restrict__ tab = tables + lab.tab_off + (in ? c : 0);
        const double hit = in ? tab[0] : kNegInf, miss = in ? tab[lab.n_cat] : kNegInf;
        const double lp = in ? tab[2 * (int64_t)lab.n_cat] : kNegInf;
        const double xc = (double)c;
#pragma unroll
        for (int k = 0; k < kJPer; ++k)
          a[k] = a[k] + (k == k_prior ? lp : (t[k].mu == xc ? hit : miss));
      }
    }
    joint_clear_past(a, i0, C);
    joint_join(a, w.m, w.s);
  }
  return w;
}

// log L of list position r from its (m, s) partials, in chunk order
// (partial[c * stride + r]); -inf when every chunk's maximum is
__device__ __forceinline__ double joint_merge(const double2* __restrict__ partial,
                                              int64_t n_chunks, int64_t stride, int64_t r) {
  double m = kNegInf;
  for (int64_t c = 0; c < n_chunks; ++c) {
    const double pm = partial[c * stride + r].x;
    m = pm > m ? pm : m;
  }
  double s = 0.0;
  for (int64_t c = 0; c < n_chunks; ++c) {
    const double2 p = partial[c * stride + r];
    s = s + (p.x == kNegInf ? 0.0 : p.y * exp(p.x - m));
  }
  return m == kNegInf ? kNegInf : m + log(s);
}
}  // namespace
}  // namespace tpe
