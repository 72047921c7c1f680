// tpe_joint_tree.hip -- the joint Parzen criterion per group of labels that
// share an activation condition (tpe.score_configs(joint="tree"); the model:
// hyperopt_amd/joint.py).  A group under a `switch` is live in
// some of a pool's rows only; its mixture is scored on those rows alone, by
// tpe_joint_score_rows (tpe_joint.hip) on a list that is made here:
//
//   tpe_rows_compact      the ascending list of the rows whose flag byte is
//                         set (one label's row of the pool's `active` block),
//                         and its length, both on the device.  Three kernels:
//                         a count per block of kCRows rows, an exclusive scan
//                         of the counts by one block (passes of kCBS counts, a
//                         running carry), and the scatter of every set row to
//                         offset[block] + its rank in the block.  Ranks and
//                         offsets are integer scans in row order
//                         (tpe_wave.hpp's block_excl_sum): no atomics, and the
//                         list does not depend on block scheduling.
//   tpe_rows_scatter      dst[rows[p]] = src[p - list_begin] over a window of
//                         that list: how score_tree_device keeps the log L_above
//                         it has just computed for a liar batch.
#include "tpe_joint.hpp"
#include "tpe_wave.hpp"

namespace tpe {
namespace {
constexpr int kCBS = 256;              // threads per compaction block
constexpr int kCPer = 8;               // consecutive rows per thread
constexpr int kCRows = kCBS * kCPer;   // rows per block

// the thread's kCPer flags as a bit mask (bit k: row first + k), rows past
// n_rows clear
__device__ __forceinline__ uint32_t flag_bits(const uint8_t* __restrict__ flags, int64_t first,
                                              int64_t n_rows) {
  uint32_t bits = 0;
#pragma unroll
  for (int k = 0; k < kCPer; ++k)
    if (first + k < n_rows && flags[first + k] != 0) bits |= 1u << k;
  return bits;
}

__global__ __launch_bounds__(kCBS) void k_compact_count(const uint8_t* __restrict__ flags,
                                                        int64_t n_rows,
                                                        int64_t* __restrict__ counts) {
  __shared__ int sh[kCBS / kWave];
  const int64_t first = ((int64_t)blockIdx.x * kCBS + threadIdx.x) * kCPer;
  int total;
  block_excl_sum<kCBS>(__popc(flag_bits(flags, first, n_rows)), sh, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// counts[b] <- the sum of counts[0, b); *out_count <- the sum of all.  One
// block; a pass of kCBS counts sums to at most kCBS * kCRows, an int.
__global__ __launch_bounds__(kCBS) void k_compact_scan(int64_t* __restrict__ counts,
                                                       int64_t n_blocks,
                                                       int64_t* __restrict__ out_count) {
  __shared__ int sh[kCBS / kWave];
  int64_t carry = 0;
  for (int64_t b0 = 0; b0 < n_blocks; b0 += kCBS) {  // (block-uniform)
    const int64_t b = b0 + threadIdx.x;
    const int c = b < n_blocks ? (int)counts[b] : 0;
    int total;
    const int before = block_excl_sum<kCBS>(c, sh, total);
    if (b < n_blocks) counts[b] = carry + before;
    carry += total;
  }
  if (threadIdx.x == 0) *out_count = carry;
}

__global__ __launch_bounds__(kCBS) void k_compact_scatter(const uint8_t* __restrict__ flags,
                                                          int64_t n_rows,
                                                          const int64_t* __restrict__ offsets,
                                                          int64_t* __restrict__ out_rows) {
  __shared__ int sh[kCBS / kWave];
  const int64_t first = ((int64_t)blockIdx.x * kCBS + threadIdx.x) * kCPer;
  const uint32_t bits = flag_bits(flags, first, n_rows);
  int total;
  const int rank = block_excl_sum<kCBS>(__popc(bits), sh, total);
  // (offset + rank + the set rows before k < the list's length <= n_rows)
  int64_t at = offsets[blockIdx.x] + rank;
#pragma unroll
  for (int k = 0; k < kCPer; ++k)
    if (bits & (1u << k)) out_rows[at++] = first + k;
}

// dst[rows[p]] = src[p - list_begin] for the list positions of the window, with
// the list scorers' guards (window_rows, tpe_joint.hpp): the count stays on the device, an entry outside
// [0, ld) is skipped
__global__ __launch_bounds__(kJBS) void k_rows_scatter(const double* __restrict__ src,
                                                       const int64_t* __restrict__ rows,
                                                       const int64_t* __restrict__ d_count,
                                                       int64_t list_begin, int64_t max_rows,
                                                       double* __restrict__ dst, int64_t ld) {
  const int64_t r = (int64_t)blockIdx.x * kJBS + threadIdx.x;
  if (r >= window_rows(d_count, list_begin, max_rows)) return;
  const int64_t row = rows[list_begin + r];
  if (row < 0 || row >= ld) return;
  dst[row] = src[r];
}

inline int64_t compact_blocks(int64_t n_rows) { return (n_rows + kCRows - 1) / kCRows; }
}  // namespace
}  // namespace tpe

using namespace tpe;

extern "C" int64_t tpe_rows_compact_scratch_bytes(int64_t n_rows) {
  if (n_rows < 0 || n_rows >= ((int64_t)1 << 40)) return -1;
  const int64_t blocks = compact_blocks(n_rows);
  return (int64_t)sizeof(int64_t) * (blocks > 0 ? blocks : 1);
}

extern "C" int tpe_rows_compact_layout(int64_t* out, int n) {
  if (out && n >= 1) out[0] = kCRows;                   // rows per block
  if (out && n >= 2) out[1] = (int64_t)kCBS * kCRows;   // rows per pass of the scan
  return 2;
}

extern "C" int tpe_rows_compact(const uint8_t* flags, int64_t n_rows, int64_t* out_rows,
                                int64_t* out_count, void* scratch, void* stream) {
  if (n_rows < 0 || n_rows >= ((int64_t)1 << 40)) {
    set_error("tpe_rows_compact: n_rows=%lld", (long long)n_rows);
    return TPE_E_ARG;
  }
  if (!out_count || !scratch || (n_rows > 0 && (!flags || !out_rows))) {
    set_error("tpe_rows_compact: null pointer");
    return TPE_E_ARG;
  }
  const int64_t blocks = compact_blocks(n_rows);  // (< 2^29)
  hipStream_t st = (hipStream_t)stream;
  int64_t* counts = static_cast<int64_t*>(scratch);
  if (blocks > 0)
    hipLaunchKernelGGL(k_compact_count, dim3((unsigned)blocks), dim3(kCBS), 0, st, flags, n_rows,
                       counts);
  hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(kCBS), 0, st, counts, blocks, out_count);
  if (blocks > 0)
    hipLaunchKernelGGL(k_compact_scatter, dim3((unsigned)blocks), dim3(kCBS), 0, st, flags,
                       n_rows, counts, out_rows);
  return check_launch("tpe_rows_compact");
}

extern "C" int tpe_rows_scatter(const double* src, const int64_t* rows, const int64_t* d_count,
                                int64_t list_begin, int64_t max_rows, double* dst, int64_t ld,
                                void* stream) {
  if (list_begin < 0 || max_rows < 0 || ld < 0 || list_begin >= ((int64_t)1 << 40) ||
      max_rows > (int64_t)2147483647 * kJBS) {
    set_error("tpe_rows_scatter: list [%lld, +%lld) ld=%lld", (long long)list_begin,
              (long long)max_rows, (long long)ld);
    return TPE_E_ARG;
  }
  if (max_rows == 0 || ld == 0) return TPE_OK;  // (ld == 0: no row is inside [0, ld))
  if (!src || !rows || !d_count || !dst) {
    set_error("tpe_rows_scatter: null pointer");
    return TPE_E_ARG;
  }
  const int64_t blocks = (max_rows + kJBS - 1) / kJBS;
  hipLaunchKernelGGL(k_rows_scatter, dim3((unsigned)blocks), dim3(kJBS), 0,
                     (hipStream_t)stream, src, rows, d_count, list_begin, max_rows, dst, ld);
  return check_launch("tpe_rows_scatter");
}
