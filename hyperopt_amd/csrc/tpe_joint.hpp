// tpe_joint.hpp -- what the joint criterion's scorer (tpe_joint.hip) and its
// sampler (tpe_joint_sample.hip) share: the layout of a prepared set, the fit
// coordinate and the label checks of the entry points.
#pragma once

#include "tpe_common.hpp"

namespace tpe {

// TPE_OK, or the error set: the labels' kinds and limits (tpe_joint.hip).
// n_tables < 0: the discrete labels' tables are not checked.
int check_joint_labels(const char* fn, const tpe_joint_label* hl, int n_labels, int n_cols,
                       int64_t n_tables);

namespace {
struct JComp {  // one (label, component) entry of a prepared set
  double mu, cst;
};

// the set buffer: log w (C) | the trial components' sigma (D) | their
// 1 / (sqrt(2) sigma) (D) | pad to an even count | JComp (D x C, label-major)
__host__ __device__ inline int64_t set_comp_off(int n_labels, int64_t C) {
  return (C + 2 * (int64_t)n_labels + 1) & ~(int64_t)1;
}

// the fit coordinate of a stored value
__device__ __forceinline__ double fit_coord(double v, bool is_log) {
  return is_log ? log(fmax(v, kEps)) : v;
}
}  // namespace
}  // namespace tpe
