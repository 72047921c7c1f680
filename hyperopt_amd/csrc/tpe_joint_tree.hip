// tpe_joint_tree.hip -- the joint Parzen criterion per group of labels that
// share an activation condition (tpe.score_configs(joint="tree"); the model:
// hyperopt_amd/joint.py).  A group under a `switch` is live in
// some of a pool's rows only; its mixture is scored on those rows alone:
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
//   tpe_joint_score_rows  tpe_joint_score with the dense row window replaced
//                         by a window of that list.  The list's length stays
//                         on the device: the grid is sized by the host's bound
//                         max_rows, and a block whose first position is at or
//                         past the length returns before it stages anything.
//                         A thread owns the row at its list position; the walk
//                         over the chunk and the merge are tpe_joint.hip's own
//                         statements (tpe_joint_pass.hpp), so log L of a row
//                         has the bits tpe_joint_score gives it.
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

// how many list positions the window [list_begin, list_begin + max_rows) holds
// (<= 0: none)
__device__ __forceinline__ int64_t window_rows(const int64_t* __restrict__ d_count,
                                               int64_t list_begin, int64_t max_rows) {
  const int64_t left = *d_count - list_begin;
  return left < max_rows ? left : max_rows;
}

__global__ __launch_bounds__(kJBS) void k_joint_score_rows(
    const tpe_joint_label* __restrict__ labels, int n_labels, const double* __restrict__ tables,
    const double* __restrict__ set, int64_t n, const double* __restrict__ vals, int64_t ld,
    const int64_t* __restrict__ rows, const int64_t* __restrict__ d_count, int64_t list_begin,
    int64_t max_rows, double2* __restrict__ partial) {
  __shared__ JComp tile[kJMaxD * kJPer];
  // block-uniform, before the first barrier: a block past the list does nothing
  const int64_t n_rows = window_rows(d_count, list_begin, max_rows);
  if ((int64_t)blockIdx.x * kJBS >= n_rows) return;
  const int64_t C = n + 1;
  const double* __restrict__ logw = set;
  const double* __restrict__ sig = set + C;
  const JComp* __restrict__ comp = reinterpret_cast<const JComp*>(set + set_comp_off(n_labels, C));
  const int64_t chunk = blockIdx.y;
  const int64_t i_first = chunk * kJChunk;
  const int64_t r = (int64_t)blockIdx.x * kJBS + threadIdx.x;  // (within the window)
  const int64_t listed = r < n_rows ? rows[list_begin + r] : -1;
  const bool live = listed >= 0 && listed < ld;
  const int64_t row = live ? listed : 0;  // (ld > 0: the entry point returns otherwise)
#define TPE_JOINT_PASS_WALK
#include "tpe_joint_pass.hpp"
  if (live) partial[chunk * max_rows + r] = double2{m, s};
}

// the merge of tpe_joint.hip's k_joint_merge, the result to out[r], out[row]
// or added to out[row]
__global__ __launch_bounds__(kJBS) void k_joint_merge_rows(
    const double2* __restrict__ partial, int64_t n_chunks, int64_t ld,
    const int64_t* __restrict__ rows, const int64_t* __restrict__ d_count, int64_t list_begin,
    int64_t max_rows, const double* __restrict__ sub, double* __restrict__ out, int out_mode) {
  const int64_t r = (int64_t)blockIdx.x * kJBS + threadIdx.x;
  if (r >= window_rows(d_count, list_begin, max_rows)) return;
  const int64_t row = rows[list_begin + r];
  if (row < 0 || row >= ld) return;
  const int64_t n_rows = max_rows;  // (the partials' stride)
#define TPE_JOINT_PASS_MERGE
#include "tpe_joint_pass.hpp"
  if (sub) v = v - sub[r];
  if (!(out_mode & TPE_JOINT_OUT_SCATTER))
    out[r] = v;
  else if (out_mode & TPE_JOINT_OUT_ADD)
    out[row] = out[row] + v;
  else
    out[row] = v;
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

extern "C" int tpe_joint_score_rows(const tpe_joint_label* host_labels,
                                    const tpe_joint_label* labels, int n_labels,
                                    const double* tables, int64_t n_tables, const double* set,
                                    int64_t n, const double* vals, int64_t ld, int n_cols,
                                    const int64_t* rows, const int64_t* d_count,
                                    int64_t list_begin, int64_t max_rows, const double* sub,
                                    double* out, int out_mode, void* scratch, void* stream) {
  const int rc = check_joint_labels("tpe_joint_score_rows", host_labels, n_labels, n_cols,
                                    n_tables < 0 ? 0 : n_tables);
  if (rc != TPE_OK) return rc;
  if (n < 0 || n >= ((int64_t)1 << 40) || list_begin < 0 || max_rows < 0 || ld < 0 ||
      list_begin >= ((int64_t)1 << 40) || max_rows >= ((int64_t)1 << 40)) {
    set_error("tpe_joint_score_rows: n=%lld list [%lld, +%lld) ld=%lld", (long long)n,
              (long long)list_begin, (long long)max_rows, (long long)ld);
    return TPE_E_ARG;
  }
  if (out_mode != 0 && out_mode != TPE_JOINT_OUT_SCATTER &&
      out_mode != (TPE_JOINT_OUT_SCATTER | TPE_JOINT_OUT_ADD)) {
    set_error("tpe_joint_score_rows: out_mode=%d", out_mode);
    return TPE_E_ARG;
  }
  if (max_rows == 0 || ld == 0) return TPE_OK;  // (ld == 0: no row is inside [0, ld))
  bool cat = false;
  for (int d = 0; d < n_labels; ++d) cat |= host_labels[d].kind == TPE_JOINT_CAT;
  if (!labels || !set || !vals || !rows || !d_count || !out || !scratch || (cat && !tables)) {
    set_error("tpe_joint_score_rows: null pointer");
    return TPE_E_ARG;
  }
  const int64_t blocks = (max_rows + kJBS - 1) / kJBS;
  const int64_t chunks = (n + 1 + kJChunk - 1) / kJChunk;
  if (blocks > 2147483647 || chunks > 65535) {
    set_error("tpe_joint_score_rows: max_rows=%lld / n=%lld do not fit a launch",
              (long long)max_rows, (long long)n);
    return TPE_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  double2* partial = static_cast<double2*>(scratch);
  hipLaunchKernelGGL(k_joint_score_rows, dim3((unsigned)blocks, (unsigned)chunks), dim3(kJBS), 0,
                     st, labels, n_labels, tables, set, n, vals, ld, rows, d_count, list_begin,
                     max_rows, partial);
  hipLaunchKernelGGL(k_joint_merge_rows, dim3((unsigned)blocks), dim3(kJBS), 0, st, partial,
                     chunks, ld, rows, d_count, list_begin, max_rows, sub, out, out_mode);
  return check_launch("tpe_joint_score_rows");
}
