// tpe_joint.hpp -- what the joint criterion's scorer (tpe_joint.hip), its
// scorer by row list (tpe_joint_tree.hip) and its sampler
// (tpe_joint_sample.hip) share: the layout of a prepared set, the fit
// coordinate, the label checks of the entry points and the scorers' constants.
// (The two scorers' one arithmetic is in tpe_joint_pass.hpp.)
#pragma once

#include "tpe_common.hpp"

namespace tpe {

// TPE_OK, or the error set: the labels' kinds and limits (tpe_joint.hip).
// n_tables < 0: the discrete labels' tables are not checked.
int check_joint_labels(const char* fn, const tpe_joint_label* hl, int n_labels, int n_cols,
                       int64_t n_tables);

namespace {
constexpr int kJBS = 256;                 // threads (rows) per block
constexpr int kJChunk = TPE_JOINT_CHUNK;  // components per partial
// components per pass, their a_i in registers: 8 gives 108 VGPRs (4 waves per
// SIMD), 16 gives 172 (2 waves), 4 gives 91 (5 waves) but half the work per
// LDS read and barrier
constexpr int kJPer = 8;
constexpr int kJMaxD = TPE_COND_MAX_LABELS;
constexpr double kNegInf = -INFINITY;
static_assert(kJChunk % kJPer == 0, "a chunk is whole passes");

// log of a component's mass of [tl, tu], -inf when it has none.  Not inlined:
// the erf and log bodies bring some forty fp64 constants that the compiler
// otherwise keeps in registers across the whole scoring loop.
__device__ __noinline__ double log_mass(double tu, double tl, double mu, double sigma) {
  const double mass = normal_cdf(tu, mu, sigma) - normal_cdf(tl, mu, sigma);
  return mass > 0.0 ? log(mass) : kNegInf;
}

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
