// tpe_joint_lie.hpp -- what the liar batches share (tpe_joint_lie.hip: one lie
// per pick over the always-live labels; tpe_joint_lie_tree.hip: one lie per
// group the pick is live in; tpe_joint_lie_chain.hip: one per chain fit, in its
// mixture and its context marginal): the control word a pick's row travels in,
// the exact (key, row) minimum of a block, the one-block kernel that turns the
// blocks' bests into the pick, and the factor of one record under a pick
// (the tree's and the chain's walks).
#pragma once

#include "tpe_joint.hpp"

namespace tpe {
namespace {
struct LieCtl {
  int64_t cur;  // the row of the last pick; -1: none was left
  int64_t pad_;
};

struct LieBest {
  uint64_t key;
  int64_t row;  // -1: no row
};

__device__ __forceinline__ uint64_t lie_key(double v) { return ~order_key(v); }

// a precedes b in (key, row) order; a missing row precedes nothing
__device__ __forceinline__ bool lie_before(const LieBest& a, const LieBest& b) {
  return a.row >= 0 && (b.row < 0 || a.key < b.key || (a.key == b.key && a.row < b.row));
}

// the block's first entry in (key, row) order, in thread 0
__device__ __forceinline__ LieBest lie_block_best(LieBest mine, LieBest* sb) {
  sb[threadIdx.x] = mine;
  __syncthreads();
  for (int off = kJBS / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off && lie_before(sb[threadIdx.x + off], sb[threadIdx.x]))
      sb[threadIdx.x] = sb[threadIdx.x + off];
    __syncthreads();
  }
  return sb[0];
}

__global__ __launch_bounds__(kJBS) void k_lie_final(const LieBest* __restrict__ partial,
                                                    int64_t n_blocks, int64_t j,
                                                    const double* __restrict__ Sw,
                                                    uint8_t* __restrict__ mask,
                                                    LieCtl* __restrict__ ctl,
                                                    int64_t* __restrict__ out_rows,
                                                    int64_t* __restrict__ out_count,
                                                    double* __restrict__ S_at_pick) {
  __shared__ LieBest sb[kJBS];
  // (no row was left for the pick before: the partials are the ones that said so)
  if (j > 0 && ctl->cur < 0) return;
  LieBest mine{0, -1};
  for (int64_t b = threadIdx.x; b < n_blocks; b += kJBS) {
    const LieBest p = partial[b];
    if (lie_before(p, mine)) mine = p;
  }
  const LieBest best = lie_block_best(mine, sb);
  if (threadIdx.x == 0) {
    ctl->cur = best.row;
    if (best.row >= 0) {
      out_rows[j] = best.row;
      if (S_at_pick) S_at_pick[j] = Sw[best.row];
      mask[best.row] = 1;
      *out_count = j + 1;
    }
  }
}

// log k_d of the stored value x under the pick's pair t: the factor
// expressions of tpe_joint_pass.hpp for one trial component, as k_lie_update
// has them.  sig is read for a label with a bandwidth only: it may be NULL
// when every label is discrete.
__device__ __forceinline__ double lie_factor(const tpe_joint_label& lab, double x, const JComp t,
                                             const double* __restrict__ sig, int d, int n_labels,
                                             const double* __restrict__ tables) {
  if (lab.kind == TPE_JOINT_CONT) {
    const double tx = fit_coord(x, (lab.flags & TPE_JOINT_LOG) != 0);
    const double u = (tx - t.mu) * sig[n_labels + d];
    return fma(-u, u, t.cst);
  }
  if (lab.kind == TPE_JOINT_QUANT) {
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
    return log_mass(tu, tl, t.mu, sig[d]) + t.cst;
  }
  const int64_t q = llrint(x);
  const bool in = q >= 0 && q < lab.n_cat;  // (a validated pool: always)
  const double* __restrict__ tab = tables + lab.tab_off + (in ? q : 0);
  const double hit = in ? tab[0] : kNegInf, miss = in ? tab[lab.n_cat] : kNegInf;
  return t.mu == (double)q ? hit : miss;
}

static_assert(sizeof(LieBest) == 16 && sizeof(LieCtl) == 16, "the scratch stays 16-byte aligned");
}  // namespace
}  // namespace tpe
