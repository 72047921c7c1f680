// tpe_joint_chain.hip -- a group's joint mixture conditioned on its context
// (tpe.score_configs(joint="chain"); the model: hyperopt_amd/joint.py "Chains",
// DESIGN 3.5.9).  The set is a mixture over the labels ctx + g, the n_ctx
// context labels first.  A row's term needs two log-sum-exps over the same
// components:
//
//   log L      over a_i     = log w_i + sum of all n_labels factors
//   log L_ctx  over a_i^ctx = log w_i + sum of the first n_ctx factors
//
// and a_i^ctx is what the walk over the labels holds in its registers when it
// reaches label n_ctx.  So both come from one walk:
//
//   tpe_joint_chain_rows  tpe_joint_score_rows (tpe_joint_tree.hip: a window
//                         of a device list of rows, a thread per row, a block
//                         per 256 rows x one chunk of components) whose walk
//                         joins the pass's a[] into a second running (m, s) at
//                         the label boundary and goes on (tpe_joint_pass.hpp
//                         under TPE_JOINT_PASS_CTX).  Two double2 partials per
//                         row and chunk; the merge forms both values in chunk
//                         order and writes log L - log L_ctx (- sub).
//
// Scoring the context by itself (tpe_joint_score_rows with n_labels = n_ctx)
// and the whole list by itself gives the same two values bit for bit, at
// n_ctx + n_labels factor evaluations per row and component in place of
// n_labels.  No atomics: a row's bits depend on the row, the set and n_ctx.
#include "tpe_joint.hpp"

namespace tpe {
namespace {
// (tpe_joint_tree.hip's: how many list positions the window holds, <= 0: none)
__device__ __forceinline__ int64_t chain_window_rows(const int64_t* __restrict__ d_count,
                                                     int64_t list_begin, int64_t max_rows) {
  const int64_t left = *d_count - list_begin;
  return left < max_rows ? left : max_rows;
}

inline int64_t chain_chunks(int64_t n) { return (n + 1 + kJChunk - 1) / kJChunk; }

// partial: [part][chunk][max_rows], part 0 the full mixture, part 1 the context's
__global__ __launch_bounds__(kJBS) void k_joint_chain_rows(
    const tpe_joint_label* __restrict__ labels, int n_labels, int n_ctx,
    const double* __restrict__ tables, const double* __restrict__ set, int64_t n,
    const double* __restrict__ vals, int64_t ld, const int64_t* __restrict__ rows,
    const int64_t* __restrict__ d_count, int64_t list_begin, int64_t max_rows,
    double2* __restrict__ partial) {
  __shared__ JComp tile[kJMaxD * kJPer];
  // block-uniform, before the first barrier: a block past the list does nothing
  const int64_t n_rows = chain_window_rows(d_count, list_begin, max_rows);
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
  double m_ctx = kNegInf, s_ctx = 0.0;
#define TPE_JOINT_PASS_CTX
#define TPE_JOINT_PASS_WALK
#include "tpe_joint_pass.hpp"
#undef TPE_JOINT_PASS_CTX
  if (live) {
    partial[chunk * max_rows + r] = double2{m, s};
    partial[((int64_t)gridDim.y + chunk) * max_rows + r] = double2{m_ctx, s_ctx};
  }
}

// both values by tpe_joint_pass.hpp's merge; (log L - log L_ctx) - sub[r] to
// out[r], out[row] or added to out[row]
__global__ __launch_bounds__(kJBS) void k_joint_chain_merge(
    const double2* __restrict__ parts, int64_t n_chunks, int64_t ld,
    const int64_t* __restrict__ rows, const int64_t* __restrict__ d_count, int64_t list_begin,
    int64_t max_rows, const double* __restrict__ sub, double* __restrict__ out, int out_mode) {
  const int64_t r = (int64_t)blockIdx.x * kJBS + threadIdx.x;
  if (r >= chain_window_rows(d_count, list_begin, max_rows)) return;
  const int64_t row = rows[list_begin + r];
  if (row < 0 || row >= ld) return;
  const int64_t n_rows = max_rows;  // (the partials' stride)
  double v_full, v_ctx;
  {
    const double2* __restrict__ partial = parts;
#define TPE_JOINT_PASS_MERGE
#include "tpe_joint_pass.hpp"
    v_full = v;
  }
  {
    const double2* __restrict__ partial = parts + n_chunks * max_rows;
#define TPE_JOINT_PASS_MERGE
#include "tpe_joint_pass.hpp"
    v_ctx = v;
  }
  double v = v_full - v_ctx;
  if (sub) v = v - sub[r];
  if (!(out_mode & TPE_JOINT_OUT_SCATTER))
    out[r] = v;
  else if (out_mode & TPE_JOINT_OUT_ADD)
    out[row] = out[row] + v;
  else
    out[row] = v;
}
}  // namespace
}  // namespace tpe

using namespace tpe;

extern "C" int64_t tpe_joint_chain_scratch_bytes(int64_t n_rows, int64_t n) {
  if (n_rows < 0 || n < 0 || n >= ((int64_t)1 << 40)) return -1;
  return 2 * (int64_t)sizeof(double2) * n_rows * chain_chunks(n);
}

extern "C" int tpe_joint_chain_rows(const tpe_joint_label* host_labels,
                                    const tpe_joint_label* labels, int n_labels, int n_ctx,
                                    const double* tables, int64_t n_tables, const double* set,
                                    int64_t n, const double* vals, int64_t ld, int n_cols,
                                    const int64_t* rows, const int64_t* d_count,
                                    int64_t list_begin, int64_t max_rows, const double* sub,
                                    double* out, int out_mode, void* scratch, void* stream) {
  const int rc = check_joint_labels("tpe_joint_chain_rows", host_labels, n_labels, n_cols,
                                    n_tables < 0 ? 0 : n_tables);
  if (rc != TPE_OK) return rc;
  if (n_ctx <= 0 || n_ctx >= n_labels) {
    set_error("tpe_joint_chain_rows: n_ctx=%d of %d labels", n_ctx, n_labels);
    return TPE_E_ARG;
  }
  if (n < 0 || n >= ((int64_t)1 << 40) || list_begin < 0 || max_rows < 0 || ld < 0 ||
      list_begin >= ((int64_t)1 << 40) || max_rows >= ((int64_t)1 << 40)) {
    set_error("tpe_joint_chain_rows: n=%lld list [%lld, +%lld) ld=%lld", (long long)n,
              (long long)list_begin, (long long)max_rows, (long long)ld);
    return TPE_E_ARG;
  }
  if (out_mode != 0 && out_mode != TPE_JOINT_OUT_SCATTER &&
      out_mode != (TPE_JOINT_OUT_SCATTER | TPE_JOINT_OUT_ADD)) {
    set_error("tpe_joint_chain_rows: out_mode=%d", out_mode);
    return TPE_E_ARG;
  }
  if (max_rows == 0 || ld == 0) return TPE_OK;  // (ld == 0: no row is inside [0, ld))
  bool cat = false;
  for (int d = 0; d < n_labels; ++d) cat |= host_labels[d].kind == TPE_JOINT_CAT;
  if (!labels || !set || !vals || !rows || !d_count || !out || !scratch || (cat && !tables)) {
    set_error("tpe_joint_chain_rows: null pointer");
    return TPE_E_ARG;
  }
  const int64_t blocks = (max_rows + kJBS - 1) / kJBS;
  const int64_t chunks = chain_chunks(n);
  if (blocks > 2147483647 || chunks > 65535) {
    set_error("tpe_joint_chain_rows: max_rows=%lld / n=%lld do not fit a launch",
              (long long)max_rows, (long long)n);
    return TPE_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  double2* partial = static_cast<double2*>(scratch);
  hipLaunchKernelGGL(k_joint_chain_rows, dim3((unsigned)blocks, (unsigned)chunks), dim3(kJBS), 0,
                     st, labels, n_labels, n_ctx, tables, set, n, vals, ld, rows, d_count,
                     list_begin, max_rows, partial);
  hipLaunchKernelGGL(k_joint_chain_merge, dim3((unsigned)blocks), dim3(kJBS), 0, st, partial,
                     chunks, ld, rows, d_count, list_begin, max_rows, sub, out, out_mode);
  return check_launch("tpe_joint_chain_rows");
}
