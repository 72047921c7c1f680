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
//                    registers (joint_walk, tpe_joint_pass.hpp).  Its running
//                    (m, s) over the chunk goes to scratch; a second kernel
//                    merges a row's chunks in chunk order (joint_merge).
//   tpe_joint_score_rows   the same over a window of a device list of rows
//                    (tpe_rows_compact, tpe_joint_tree.hip).  The
//                    list's length stays on the device: the grid is sized by
//                    the host's bound max_rows, and a block whose first
//                    position is at or past the length returns before it
//                    stages anything.  A thread owns the row at its list
//                    position.
//   tpe_joint_chain_rows   the list scorer for a group's mixture conditioned on
//                    its context (joint="chain").  The set is a
//                    mixture over the labels ctx + g, the n_ctx context labels
//                    first.  A row's term is log L - log L_ctx: log L over the
//                    a_i of all n_labels factors, log L_ctx over the a_i of the
//                    first n_ctx, which is what the walk holds in its registers
//                    when it reaches label n_ctx.  So one walk gives both: two
//                    double2 partials per row and chunk, and the merge forms
//                    both values in chunk order.  Scoring the context by itself
//                    (n_labels = n_ctx) and the whole list by itself gives the
//                    same two values bit for bit, at n_ctx + n_labels factor
//                    evaluations per row and component in place of n_labels.
//
// Flat is tree with one group, tree is chain with an empty context: the three
// entries are one walk kernel and one merge kernel, k_joint_rows<kList, kCtx>
// and k_joint_rows_merge<kList, kCtx>, instantiated <false, false> (a dense
// window), <true, false> (a list) and <true, true> (a list and a context), and
// one host driver (joint_rows).
//
// A row's bits depend on the row, the set, n_ctx and kJChunk / kJPer only: a
// thread owns its row alone, every sum has a fixed order, there are no
// atomics, and the window or the list only moves the row to another thread.
#include "tpe_joint_pass.hpp"

namespace tpe {
namespace {
// (kJBS, kJChunk, kJPer, kJMaxD, log_mass, JComp, set_comp_off, fit_coord,
// joint_chunks and window_rows: tpe_joint.hpp.)

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

// The walk.  A window of n_rows positions from `begin`: of the pool's rows
// (kList false: position r is row begin + r), or of the device list `rows` of
// *d_count entries (kList: position r is row rows[begin + r]; an entry outside
// [0, ld) is skipped).  partial: [part][chunk][n_rows], part 0 the full
// mixture, part 1 (kCtx) the context's.
template <bool kList, bool kCtx>
__global__ __launch_bounds__(kJBS) void k_joint_rows(
    const tpe_joint_label* __restrict__ labels, int n_labels, int n_ctx,
    const double* __restrict__ tables, const double* __restrict__ set, int64_t n,
    const double* __restrict__ vals, int64_t ld, const int64_t* __restrict__ rows,
    const int64_t* __restrict__ d_count, int64_t begin, int64_t n_rows,
    double2* __restrict__ partial) {
  __shared__ JComp tile[kJMaxD * kJPer];
  const int64_t chunk = blockIdx.y;
  const int64_t r = (int64_t)blockIdx.x * kJBS + threadIdx.x;  // (within the window)
  bool live;
  int64_t row;
  if constexpr (kList) {
    // block-uniform, before the first barrier: a block past the list does nothing
    const int64_t listed_rows = window_rows(d_count, begin, n_rows);
    if ((int64_t)blockIdx.x * kJBS >= listed_rows) return;
    const int64_t listed = r < listed_rows ? rows[begin + r] : -1;
    live = listed >= 0 && listed < ld;
    row = live ? listed : 0;  // (ld > 0: the entry point returns otherwise)
  } else {
    live = r < n_rows;
    row = begin + (live ? r : 0);
  }
  const JWalk w = joint_walk<kCtx>(labels, n_labels, n_ctx, tables, set, n, vals, ld, row,
                                   chunk * kJChunk, tile);
  if (!live) return;
  partial[chunk * n_rows + r] = double2{w.m, w.s};
  if constexpr (kCtx)
    partial[((int64_t)gridDim.y + chunk) * n_rows + r] = double2{w.m_ctx, w.s_ctx};
}

// The merge: v = log L of position r from its partials in chunk order; with a
// context v = log L - log L_ctx, and the two values themselves go to
// keep_full[row] / keep_ctx[row] where given (row < keep_ld).  v - sub[r] to
// out[r], out[row] or added to out[row] (out_mode; a dense window: out[r]).
template <bool kList, bool kCtx>
__global__ __launch_bounds__(kJBS) void k_joint_rows_merge(
    const double2* __restrict__ partial, int64_t n_chunks, int64_t ld,
    const int64_t* __restrict__ rows, const int64_t* __restrict__ d_count, int64_t begin,
    int64_t n_rows, const double* __restrict__ sub, double* __restrict__ out, int out_mode,
    double* __restrict__ keep_full, double* __restrict__ keep_ctx, int64_t keep_ld) {
  const int64_t r = (int64_t)blockIdx.x * kJBS + threadIdx.x;
  int64_t row = r;
  if constexpr (kList) {
    if (r >= window_rows(d_count, begin, n_rows)) return;
    row = rows[begin + r];
    if (row < 0 || row >= ld) return;
  } else {
    if (r >= n_rows) return;
  }
  double v = joint_merge(partial, n_chunks, n_rows, r);
  if constexpr (kCtx) {
    const double v_ctx = joint_merge(partial + n_chunks * n_rows, n_chunks, n_rows, r);
    if (row < keep_ld) {
      if (keep_full) keep_full[row] = v;
      if (keep_ctx) keep_ctx[row] = v_ctx;
    }
    v = v - v_ctx;
  }
  if (sub) v = v - sub[r];
  if (!(out_mode & TPE_JOINT_OUT_SCATTER))
    out[r] = v;
  else if (out_mode & TPE_JOINT_OUT_ADD)
    out[row] = out[row] + v;
  else
    out[row] = v;
}

// one scoring call: the arguments of the three entry points
struct JointRows {
  const char* fn;  // the entry's name in error texts
  const tpe_joint_label *host_labels, *labels;
  int n_labels;
  bool ctx;   // the first n_ctx labels are a context (n_ctx in (0, n_labels))
  int n_ctx;
  const double* tables;
  int64_t n_tables;
  const double* set;
  int64_t n;
  const double* vals;
  int64_t ld;
  int n_cols;
  bool list;  // rows / d_count are a device list, begin a position in it
  const int64_t *rows, *d_count;
  int64_t begin, n_rows;
  const double* sub;
  double* out;
  int out_mode;
  double *keep_full, *keep_ctx;
  int64_t keep_ld;
  void *scratch, *stream;
};

template <bool kList, bool kCtx>
void launch_joint_rows(const JointRows& a, int64_t blocks, int64_t chunks) {
  hipStream_t st = (hipStream_t)a.stream;
  double2* partial = static_cast<double2*>(a.scratch);
  hipLaunchKernelGGL((k_joint_rows<kList, kCtx>), dim3((unsigned)blocks, (unsigned)chunks),
                     dim3(kJBS), 0, st, a.labels, a.n_labels, a.n_ctx, a.tables, a.set, a.n, a.vals,
                     a.ld, a.rows, a.d_count, a.begin, a.n_rows, partial);
  hipLaunchKernelGGL((k_joint_rows_merge<kList, kCtx>), dim3((unsigned)blocks), dim3(kJBS), 0, st,
                     partial, chunks, a.ld, a.rows, a.d_count, a.begin, a.n_rows, a.sub, a.out,
                     a.out_mode, a.keep_full, a.keep_ctx,
                     a.keep_full || a.keep_ctx ? a.keep_ld : 0);
}

// validates once, launches once
int joint_rows(const JointRows& a) {
  const int rc = check_joint_labels(a.fn, a.host_labels, a.n_labels, a.n_cols,
                                    a.n_tables < 0 ? 0 : a.n_tables);
  if (rc != TPE_OK) return rc;
  if ((a.keep_full || a.keep_ctx) && a.keep_ld < 0) {
    set_error("%s_keep: keep_ld=%lld", a.fn, (long long)a.keep_ld);
    return TPE_E_ARG;
  }
  if (a.ctx && (a.n_ctx <= 0 || a.n_ctx >= a.n_labels)) {
    set_error("%s: n_ctx=%d of %d labels", a.fn, a.n_ctx, a.n_labels);
    return TPE_E_ARG;
  }
  // a dense window lies inside the pool; a list's entries are checked on the device
  const bool range = a.list ? a.begin < ((int64_t)1 << 40) && a.n_rows < ((int64_t)1 << 40)
                            : a.begin <= a.ld && a.n_rows <= a.ld - a.begin;
  if (a.n < 0 || a.n >= ((int64_t)1 << 40) || a.begin < 0 || a.n_rows < 0 || a.ld < 0 || !range) {
    set_error("%s: n=%lld %s [%lld, +%lld) ld=%lld", a.fn, (long long)a.n,
              a.list ? "list" : "rows", (long long)a.begin, (long long)a.n_rows, (long long)a.ld);
    return TPE_E_ARG;
  }
  if (a.out_mode != 0 && a.out_mode != TPE_JOINT_OUT_SCATTER &&
      a.out_mode != (TPE_JOINT_OUT_SCATTER | TPE_JOINT_OUT_ADD)) {
    set_error("%s: out_mode=%d", a.fn, a.out_mode);
    return TPE_E_ARG;
  }
  if (a.n_rows == 0 || (a.list && a.ld == 0)) return TPE_OK;  // (ld == 0: no listed row is inside)
  bool cat = false;
  for (int d = 0; d < a.n_labels; ++d) cat |= a.host_labels[d].kind == TPE_JOINT_CAT;
  if (!a.labels || !a.set || !a.vals || !a.out || !a.scratch || (cat && !a.tables) ||
      (a.list && (!a.rows || !a.d_count))) {
    set_error("%s: null pointer", a.fn);
    return TPE_E_ARG;
  }
  const int64_t blocks = (a.n_rows + kJBS - 1) / kJBS, chunks = joint_chunks(a.n);
  if (blocks > 2147483647 || chunks > 65535) {
    set_error("%s: n_rows=%lld / n=%lld do not fit a launch", a.fn, (long long)a.n_rows,
              (long long)a.n);
    return TPE_E_ARG;
  }
  if (a.ctx)
    launch_joint_rows<true, true>(a, blocks, chunks);
  else if (a.list)
    launch_joint_rows<true, false>(a, blocks, chunks);
  else
    launch_joint_rows<false, false>(a, blocks, chunks);
  return check_launch(a.fn);
}
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

extern "C" int64_t tpe_joint_chain_scratch_bytes(int64_t n_rows, int64_t n) {
  const int64_t one = tpe_joint_scratch_bytes(n_rows, n);
  return one < 0 ? -1 : 2 * one;
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
  return joint_rows({"tpe_joint_score", host_labels, labels, n_labels, false, 0, tables, n_tables,
                     set, n, vals, ld, n_cols, false, nullptr, nullptr, row_begin, n_rows, sub, out,
                     0, nullptr, nullptr, 0, scratch, stream});
}

extern "C" int tpe_joint_score_rows(const tpe_joint_label* host_labels,
                                    const tpe_joint_label* labels, int n_labels,
                                    const double* tables, int64_t n_tables, const double* set,
                                    int64_t n, const double* vals, int64_t ld, int n_cols,
                                    const int64_t* rows, const int64_t* d_count,
                                    int64_t list_begin, int64_t max_rows, const double* sub,
                                    double* out, int out_mode, void* scratch, void* stream) {
  return joint_rows({"tpe_joint_score_rows", host_labels, labels, n_labels, false, 0, tables,
                     n_tables, set, n, vals, ld, n_cols, true, rows, d_count, list_begin, max_rows,
                     sub, out, out_mode, nullptr, nullptr, 0, scratch, stream});
}

// (reports as tpe_joint_chain_rows)
extern "C" int tpe_joint_chain_rows_keep(
    const tpe_joint_label* host_labels, const tpe_joint_label* labels, int n_labels, int n_ctx,
    const double* tables, int64_t n_tables, const double* set, int64_t n, const double* vals,
    int64_t ld, int n_cols, const int64_t* rows, const int64_t* d_count, int64_t list_begin,
    int64_t max_rows, const double* sub, double* out, int out_mode, double* keep_full,
    double* keep_ctx, int64_t keep_ld, void* scratch, void* stream) {
  return joint_rows({"tpe_joint_chain_rows", host_labels, labels, n_labels, true, n_ctx, tables,
                     n_tables, set, n, vals, ld, n_cols, true, rows, d_count, list_begin, max_rows,
                     sub, out, out_mode, keep_full, keep_ctx, keep_ld, scratch, stream});
}

extern "C" int tpe_joint_chain_rows(const tpe_joint_label* host_labels,
                                    const tpe_joint_label* labels, int n_labels, int n_ctx,
                                    const double* tables, int64_t n_tables, const double* set,
                                    int64_t n, const double* vals, int64_t ld, int n_cols,
                                    const int64_t* rows, const int64_t* d_count,
                                    int64_t list_begin, int64_t max_rows, const double* sub,
                                    double* out, int out_mode, void* scratch, void* stream) {
  return tpe_joint_chain_rows_keep(host_labels, labels, n_labels, n_ctx, tables, n_tables, set, n,
                                   vals, ld, n_cols, rows, d_count, list_begin, max_rows, sub, out,
                                   out_mode, nullptr, nullptr, 0, scratch, stream);
}

extern "C" int tpe_joint_struct_sizes(int32_t* out, int n) {
  if (out && n >= 1) out[0] = (int32_t)sizeof(tpe_joint_label);
  return 1;
}
