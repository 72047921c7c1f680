// tpe_joint.hip -- a joint (multivariate) Parzen criterion over a pool's rows
// (tpe.score_configs(joint=True); the model: hyperopt_amd/joint.py, DESIGN
// 3.5.4).
//
// One set (below or above) is a mixture of C = n + 1 product kernels over the
// D joint labels: one per trial of the set, in row order, and the prior last.
// For a pool row c
//
//   a_i      = log w_i + sum_d log k_{d,i}(c_d)     (d in list order, from log w_i)
//   log L(c) = m + log sum_i exp(a_i - m),  m = max_i a_i   (-inf when m is)
//
//   tpe_joint_prep   the set's components from the history in HBM: per (label,
//                    component) the pair {mu, constant} -- mu the observation
//                    in the fit coordinate (log max(x, EPS) for the log kinds;
//                    the category for a discrete label), the constant
//                    -log(sigma sqrt(2 pi)) - log Z (a quantized label: -log Z).
//   tpe_joint_score  log L of a window of pool rows.  The components are cut
//                    into chunks of kJChunk (compile time); a block is 256 rows
//                    x one chunk, a thread one row.  The thread walks the chunk
//                    in passes of kJPer components whose a_i it keeps in
//                    registers: labels outside, components inside, the pass's
//                    {mu, constant} pairs staged in LDS and read as broadcasts.
//                    Its running (m, s) over the chunk goes to scratch; a second
//                    kernel merges a row's chunks in chunk order.
//
// A row's bits depend on the row, the set and kJChunk / kJPer only: a thread
// owns its row alone, every sum has a fixed order, there are no atomics, and
// the row window only moves the row to another thread.
#include "tpe_joint.hpp"

namespace tpe {
namespace {
// (kJBS, kJChunk, kJPer, kJMaxD, log_mass, JComp, set_comp_off and fit_coord:
// tpe_joint.hpp.  The walk over a chunk and the merge, which the list scorer
// of tpe_joint_tree.hip shares: tpe_joint_pass.hpp, included below as text.)

// thread (i, d): component i of label d
__global__ __launch_bounds__(kJBS) void k_joint_prep(const tpe_joint_label* __restrict__ labels,
                                                     int n_labels,
                                                     const double* __restrict__ hvals,
                                                     const uint8_t* __restrict__ hact,
                                                     int64_t hld,
                                                     const int32_t* __restrict__ rows, int64_t n,
                                                     double* __restrict__ set) {
  const int64_t C = n + 1;
  const int64_t i = (int64_t)blockIdx.x * kJBS + threadIdx.x;
  const int d = blockIdx.y;
  if (i >= C) return;
  const tpe_joint_label lab = labels[d];
  const bool is_log = (lab.flags & TPE_JOINT_LOG) != 0;
  double mu, sigma;
  if (i < n) {
    const int64_t row = rows ? (int64_t)rows[i] : i;
    const int64_t e = (int64_t)lab.col * hld + row;
    const bool ok = row >= 0 && row < hld && hact[e] != 0;
    const double v = ok ? hvals[e] - lab.shift : __longlong_as_double(0x7FF8000000000000ll);
    mu = lab.kind == TPE_JOINT_CAT ? (double)llrint(v) : fit_coord(v, is_log);
    sigma = set[C + d];
  } else {
    mu = lab.kind == TPE_JOINT_CAT ? -1.0 : lab.prior_mu;
    sigma = lab.prior_sigma;
  }
  double cst = 0.0;
  if (lab.kind != TPE_JOINT_CAT) {
    if (lab.flags & TPE_JOINT_BOUNDED)
      cst = -log(normal_cdf(lab.hi, mu, sigma) - normal_cdf(lab.lo, mu, sigma));
    if (lab.kind == TPE_JOINT_CONT) cst = -log(sigma * sqrt(kTwoPi)) + cst;
  }
  JComp* comp = reinterpret_cast<JComp*>(set + set_comp_off(n_labels, C));
  comp[(int64_t)d * C + i] = JComp{mu, cst};
}

__global__ __launch_bounds__(kJBS) void k_joint_score(const tpe_joint_label* __restrict__ labels,
                                                      int n_labels,
                                                      const double* __restrict__ tables,
                                                      const double* __restrict__ set, int64_t n,
                                                      const double* __restrict__ vals, int64_t ld,
                                                      int64_t row_begin, int64_t n_rows,
                                                      double2* __restrict__ partial) {
  __shared__ JComp tile[kJMaxD * kJPer];
  const int64_t C = n + 1;
  const double* __restrict__ logw = set;
  const double* __restrict__ sig = set + C;
  const JComp* __restrict__ comp = reinterpret_cast<const JComp*>(set + set_comp_off(n_labels, C));
  const int64_t chunk = blockIdx.y;
  const int64_t i_first = chunk * kJChunk;
  const int64_t r = (int64_t)blockIdx.x * kJBS + threadIdx.x;  // (within the window)
  const bool live = r < n_rows;
  const int64_t row = row_begin + (live ? r : 0);
#define TPE_JOINT_PASS_WALK
#include "tpe_joint_pass.hpp"
  if (live) partial[chunk * n_rows + r] = double2{m, s};
}

// out[r] = log L from the row's partials in chunk order, minus sub[r]
__global__ __launch_bounds__(kJBS) void k_joint_merge(const double2* __restrict__ partial,
                                                      int64_t n_chunks, int64_t n_rows,
                                                      const double* __restrict__ sub,
                                                      double* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * kJBS + threadIdx.x;
  if (r >= n_rows) return;
#define TPE_JOINT_PASS_MERGE
#include "tpe_joint_pass.hpp"
  if (sub) v = v - sub[r];
  out[r] = v;
}

inline int64_t joint_chunks(int64_t n) { return (n + 1 + kJChunk - 1) / kJChunk; }
}  // namespace

// TPE_OK, or the error set: the labels' kinds and limits (shared with the
// sampler: tpe_joint.hpp)
int check_joint_labels(const char* fn, const tpe_joint_label* hl, int n_labels, int n_cols,
                       int64_t n_tables) {
  if (n_labels <= 0 || !hl) {
    set_error("%s: n_labels=%d / null labels", fn, n_labels);
    return TPE_E_ARG;
  }
  if (n_labels > kJMaxD) {
    set_error("%s: %d joint labels, at most %d", fn, n_labels, kJMaxD);
    return TPE_E_UNSUPPORTED;
  }
  for (int d = 0; d < n_labels; ++d) {
    const tpe_joint_label& l = hl[d];
    if (l.kind < TPE_JOINT_CONT || l.kind > TPE_JOINT_CAT || l.col < 0 || l.col >= n_cols ||
        (l.kind == TPE_JOINT_CAT && (l.n_cat <= 0 || l.tab_off < 0)) ||
        (l.kind == TPE_JOINT_QUANT && !(l.q > 0.0))) {
      set_error("%s: label %d: kind=%d col=%d n_cat=%d q=%g", fn, d, l.kind, l.col, l.n_cat, l.q);
      return TPE_E_ARG;
    }
    if (l.kind == TPE_JOINT_CAT && l.n_cat > TPE_JOINT_MAX_CAT) {
      set_error("%s: label %d has %d options, at most %d", fn, d, l.n_cat, TPE_JOINT_MAX_CAT);
      return TPE_E_UNSUPPORTED;
    }
    if (l.kind == TPE_JOINT_CAT && n_tables >= 0 && l.tab_off + 3 * (int64_t)l.n_cat > n_tables) {
      set_error("%s: label %d: its tables end at %lld of %lld", fn, d,
                (long long)(l.tab_off + 3 * (int64_t)l.n_cat), (long long)n_tables);
      return TPE_E_ARG;
    }
  }
  return TPE_OK;
}
}  // namespace tpe

using namespace tpe;

extern "C" int tpe_joint_chunk(void) { return kJChunk; }

extern "C" int64_t tpe_joint_set_doubles(int n_labels, int64_t n) {
  if (n_labels < 0 || n < 0 || n >= ((int64_t)1 << 40)) return -1;
  return set_comp_off(n_labels, n + 1) + 2 * (int64_t)n_labels * (n + 1);
}

extern "C" int64_t tpe_joint_scratch_bytes(int64_t n_rows, int64_t n) {
  if (n_rows < 0 || n < 0 || n >= ((int64_t)1 << 40)) return -1;
  return (int64_t)sizeof(double2) * n_rows * joint_chunks(n);
}

extern "C" int tpe_joint_prep(const tpe_joint_label* host_labels, const tpe_joint_label* labels,
                              int n_labels, const double* hist_vals, const uint8_t* hist_active,
                              int64_t hist_ld, int hist_cols, const int32_t* rows, int64_t n,
                              double* set, void* stream) {
  const int rc = check_joint_labels("tpe_joint_prep", host_labels, n_labels, hist_cols, -1);
  if (rc != TPE_OK) return rc;
  if (n < 0 || hist_ld < 0 || (!rows && n > hist_ld) || n >= ((int64_t)1 << 40)) {
    set_error("tpe_joint_prep: n=%lld hist_ld=%lld", (long long)n, (long long)hist_ld);
    return TPE_E_ARG;
  }
  if (!labels || !set || (n > 0 && (!hist_vals || !hist_active))) {
    set_error("tpe_joint_prep: null pointer");
    return TPE_E_ARG;
  }
  const dim3 grid((unsigned)((n + 1 + kJBS - 1) / kJBS), (unsigned)n_labels);
  hipLaunchKernelGGL(k_joint_prep, grid, dim3(kJBS), 0, (hipStream_t)stream, labels, n_labels,
                     hist_vals, hist_active, hist_ld, rows, n, set);
  return check_launch("tpe_joint_prep");
}

extern "C" int tpe_joint_score(const tpe_joint_label* host_labels, const tpe_joint_label* labels,
                               int n_labels, const double* tables, int64_t n_tables,
                               const double* set, int64_t n, const double* vals, int64_t ld,
                               int n_cols, int64_t row_begin, int64_t n_rows, const double* sub,
                               double* out, void* scratch, void* stream) {
  const int rc = check_joint_labels("tpe_joint_score", host_labels, n_labels, n_cols,
                                    n_tables < 0 ? 0 : n_tables);
  if (rc != TPE_OK) return rc;
  if (n < 0 || n >= ((int64_t)1 << 40) || row_begin < 0 || n_rows < 0 || ld < 0 ||
      row_begin > ld || n_rows > ld - row_begin) {
    set_error("tpe_joint_score: n=%lld rows [%lld, +%lld) of ld=%lld", (long long)n,
              (long long)row_begin, (long long)n_rows, (long long)ld);
    return TPE_E_ARG;
  }
  if (n_rows == 0) return TPE_OK;
  bool cat = false;
  for (int d = 0; d < n_labels; ++d) cat |= host_labels[d].kind == TPE_JOINT_CAT;
  if (!labels || !set || !vals || !out || !scratch || (cat && !tables)) {
    set_error("tpe_joint_score: null pointer");
    return TPE_E_ARG;
  }
  const int64_t blocks = (n_rows + kJBS - 1) / kJBS, chunks = joint_chunks(n);
  if (blocks > 2147483647 || chunks > 65535) {
    set_error("tpe_joint_score: n_rows=%lld / n=%lld do not fit a launch", (long long)n_rows,
              (long long)n);
    return TPE_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  double2* partial = static_cast<double2*>(scratch);
  hipLaunchKernelGGL(k_joint_score, dim3((unsigned)blocks, (unsigned)chunks), dim3(kJBS), 0, st,
                     labels, n_labels, tables, set, n, vals, ld, row_begin, n_rows, partial);
  hipLaunchKernelGGL(k_joint_merge, dim3((unsigned)blocks), dim3(kJBS), 0, st, partial, chunks,
                     n_rows, sub, out);
  return check_launch("tpe_joint_score");
}

extern "C" int tpe_joint_struct_sizes(int32_t* out, int n) {
  if (out && n >= 1) out[0] = (int32_t)sizeof(tpe_joint_label);
  return 1;
}
