// tpe_joint_lie.hpp -- what the two liar batches share (tpe_joint_lie.hip: one
// lie per pick over the always-live labels; tpe_joint_lie_tree.hip: one lie per
// group the pick is live in): the control word a pick's row travels in, the
// exact (key, row) minimum of a block, and the one-block kernel that turns the
// blocks' bests into the pick.
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

static_assert(sizeof(LieBest) == 16 && sizeof(LieCtl) == 16, "the scratch stays 16-byte aligned");
}  // namespace
}  // namespace tpe
