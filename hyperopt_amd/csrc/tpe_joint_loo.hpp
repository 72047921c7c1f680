// tpe_joint_loo.hpp -- what the two leave-one-out selectors share
// (tpe_joint_loo.hip: one multiplier for every label; tpe_joint_loo_label.hip:
// one label's multiplier with the others held): the grid record, a bounded
// component's -log Z, the online join of an exponent and the last sum.
#pragma once

#include "tpe_joint.hpp"

namespace tpe {
namespace {
constexpr int kLMaxB = TPE_LOO_MAX_GRID;

struct LooGrid {
  double scale[kLMaxB];  // s_b = h_b n^(-1/(D+4))
  double inv[kLMaxB];    // 1 / s_b^2
};

// -log Z of a bounded label's component
__device__ __forceinline__ double neg_log_z(const tpe_joint_label& lab, double mu, double sigma) {
  return -log(normal_cdf(lab.hi, mu, sigma) - normal_cdf(lab.lo, mu, sigma));
}

// (m, s) <- (m, s) joined with the exponent a: one exp whichever is larger
__device__ __forceinline__ void loo_join(double& m, double& s, double a) {
  if (a != kNegInf) {
    const double d = a - m;  // (m = -inf: +inf, e = 0 and s, which is 0, becomes 1)
    const double e = exp(-fabs(d));
    s = d > 0.0 ? fma(s, e, 1.0) : s + e;
    m = d > 0.0 ? a : m;
  }
}

// out[b] = the block sums in block order, over sum v (no block: 0, the n < 2 rule)
__global__ void k_loo_final(const double* __restrict__ blk, int64_t n_blocks, int n_grid,
                            double sum_v, double* __restrict__ out) {
  const int b = threadIdx.x;
  if (b >= n_grid) return;
  double s = 0.0;
  for (int64_t k = 0; k < n_blocks; ++k) s = s + blk[(int64_t)b * n_blocks + k];
  out[b] = n_blocks ? s / sum_v : 0.0;
}
}  // namespace
}  // namespace tpe
