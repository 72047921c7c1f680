// tpe_joint_lie_tree.hip -- the liar batch under joint="tree": a pick lies in
// every group of labels it is live in (tpe.suggest_from_pool(joint="tree",
// batch="liar-tree"); the model: hyperopt_amd/joint.py "Batches in a tree",
// DESIGN 3.5.13).
//
// Every group g has its own above mixture, so every group keeps its own U:
//
//   U_{g,0}[r] = log W_g + A_g[r]                       (g live in r)
//   c_{g,p}(r) = log(lie_weight) + sum_{d in g} log k_d(r_d)   (g live in p and r)
//   U_{g,j}[r] = U_{g,j-1}[r] joined with c_{g,p_j}(r)  (tpe_joint_lie.hip's rule)
//   S_j[r]     = S_0[r] - sum_g (U_{g,j}[r] - U_{g,0}[r])   in group order, over
//                the groups live in r whose U_{g,0}[r] is finite
//
//   k_lie_tree_init    a thread per row: U_0 and U of the groups live in its row
//                      (group-major (G, P): a wave's accesses coalesce; places
//                      of groups not live in the row are never read), the
//                      working S and mask, the block's best free row
//   k_lie_final        tpe_joint_lie.hpp's, unchanged
//   k_lie_tree_update  256 rows per block.  The block reads the pick's row from
//                      the control word; thread g stages whether group g is live
//                      in the pick, thread d the {mu, constant} pair of label d
//                      where its group is (<= 128 x 16 B of LDS).  Then a thread
//                      per row walks the groups in order: a group not live in
//                      the row is skipped; one not live in the pick (block-
//                      uniform) costs the loads of U and U_0 and a subtract; one
//                      live in both walks its labels with the pairs as LDS
//                      broadcasts, joins U and stores it.  The penalties fold in
//                      group order into S_j, which joins the block's argmax.
//   k_rows_scatter     dst[rows[p]] = src[p - list_begin] over a window of a
//                      device list (tpe_rows_scatter): how score_tree_device
//                      keeps the log L_above it has just computed.
//
// Rows of different branches share a wave, so the group branch diverges: a wave
// executes at most the labels of the groups live in any of its rows, <= D_tot,
// the flat kernel's cost per pick.  The groups' offsets, liveness columns and
// log W travel by value in the kernel arguments (2 KiB): a group index is
// uniform, so they are scalar loads.  No floating-point atomics, a thread owns
// its row, the (key, row) minimum is exact: a row's bits depend on the row, the
// sets and the pick sequence alone.
#include "tpe_joint_lie.hpp"

namespace tpe {
namespace {
struct LieGroups {
  int n;                  // G
  int off[kJMaxD + 1];    // group g's labels: [off[g], off[g + 1])
  int col[kJMaxD];        // the column whose `active` byte says g is live; -1: always
  double log_w[kJMaxD];   // log W_g
};

__device__ __forceinline__ bool group_live(const LieGroups& grp, int g,
                                           const uint8_t* __restrict__ active, int64_t ld,
                                           int64_t row) {
  const int c = grp.col[g];
  return c < 0 || active[(int64_t)c * ld + row] != 0;
}

__global__ __launch_bounds__(kJBS) void k_lie_tree_init(
    const LieGroups grp, const double* __restrict__ S0, const double* __restrict__ A, int64_t ldA,
    const uint8_t* __restrict__ active, int64_t ld, const uint8_t* __restrict__ taken,
    const uint8_t* __restrict__ distinct, int64_t n_rows, double* __restrict__ U0,
    double* __restrict__ U, double* __restrict__ Sw, uint8_t* __restrict__ mask,
    LieBest* __restrict__ partial, LieCtl* __restrict__ ctl, int64_t* __restrict__ out_count) {
  __shared__ LieBest sb[kJBS];
  const int64_t r = (int64_t)blockIdx.x * kJBS + threadIdx.x;
  LieBest mine{0, -1};
  if (r < n_rows) {
    for (int g = 0; g < grp.n; ++g) {
      if (!group_live(grp, g, active, ld, r)) continue;
      const double u = grp.log_w[g] + A[(int64_t)g * ldA + r];
      U0[(int64_t)g * n_rows + r] = u;
      U[(int64_t)g * n_rows + r] = u;
    }
    const double s = S0[r];
    const uint8_t gone = (taken[r] != 0) | (distinct ? distinct[r] != 0 : 0);
    Sw[r] = s;
    mask[r] = gone;
    if (!gone) mine = LieBest{lie_key(s), r};
  }
  const LieBest best = lie_block_best(mine, sb);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = best;
    if (blockIdx.x == 0) {
      ctl->cur = -1;
      *out_count = 0;
    }
  }
}

__global__ __launch_bounds__(kJBS) void k_lie_tree_update(
    const LieGroups grp, const tpe_joint_label* __restrict__ labels, int n_labels,
    const double* __restrict__ tables, const double* __restrict__ sig,
    const double* __restrict__ vals, const uint8_t* __restrict__ active, int64_t ld,
    int64_t n_rows, const double* __restrict__ S0, double log_lie,
    const LieCtl* __restrict__ ctl, const double* __restrict__ U0, double* __restrict__ U,
    double* __restrict__ Sw, const uint8_t* __restrict__ mask, LieBest* __restrict__ partial) {
  __shared__ JComp pick[kJMaxD];
  __shared__ uint8_t in_pick[kJMaxD];
  __shared__ LieBest sb[kJBS];
  const int64_t p = ctl->cur;
  if (p < 0) return;  // (the whole grid: no pick, nothing to add)
  for (int g = threadIdx.x; g < grp.n; g += kJBS) in_pick[g] = group_live(grp, g, active, ld, p);
  // the pick as a trial component of each above set it is live in: what
  // k_joint_prep would write for a history row that held row p
  for (int d = threadIdx.x; d < n_labels; d += kJBS) {
    int g = 0;
    while (grp.off[g + 1] <= d) ++g;  // (off[G] = n_labels > d)
    if (!group_live(grp, g, active, ld, p)) continue;  // (its values are not row p's to read)
    const tpe_joint_label lab = labels[d];
    const double v = vals[(int64_t)lab.col * ld + p];
    double mu, cst = 0.0;
    if (lab.kind == TPE_JOINT_CAT) {
      mu = (double)llrint(v);
    } else {
      const double sigma = sig[d];
      mu = fit_coord(v, (lab.flags & TPE_JOINT_LOG) != 0);
      if (lab.flags & TPE_JOINT_BOUNDED)
        cst = -log(normal_cdf(lab.hi, mu, sigma) - normal_cdf(lab.lo, mu, sigma));
      if (lab.kind == TPE_JOINT_CONT) cst = -log(sigma * sqrt(kTwoPi)) + cst;
    }
    pick[d] = JComp{mu, cst};
  }
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * kJBS + threadIdx.x;
  LieBest mine{0, -1};
  if (r < n_rows) {
    double s = S0[r];
    for (int g = 0; g < grp.n; ++g) {
      if (!group_live(grp, g, active, ld, r)) continue;
      const int64_t at = (int64_t)g * n_rows + r;
      const double u = U[at];
      double un = u;
      if (in_pick[g]) {
        double c = log_lie;
        for (int d = grp.off[g]; d < grp.off[g + 1]; ++d) {
          const tpe_joint_label lab = labels[d];
          const double x = vals[(int64_t)lab.col * ld + r];
          c = c + lie_factor(lab, x, pick[d], sig, d, n_labels, tables);
        }
        if (c != kNegInf) {  // (c = -inf leaves U's bits)
          const double m = c > u ? c : u;
          un = m == kNegInf ? kNegInf : m + log(exp(u - m) + exp(c - m));
          U[at] = un;
        }
      }
      const double u0 = U0[at];
      if (fabs(u0) < INFINITY) s = s - (un - u0);
    }
    Sw[r] = s;
    if (!mask[r]) mine = LieBest{lie_key(s), r};
  }
  const LieBest best = lie_block_best(mine, sb);
  if (threadIdx.x == 0) partial[blockIdx.x] = best;
}

// dst[rows[p]] = src[p - list_begin] for the list positions of the window, with
// k_joint_merge_rows' guards: the count stays on the device, an entry outside
// [0, ld) is skipped
__global__ __launch_bounds__(kJBS) void k_rows_scatter(const double* __restrict__ src,
                                                       const int64_t* __restrict__ rows,
                                                       const int64_t* __restrict__ d_count,
                                                       int64_t list_begin, int64_t max_rows,
                                                       double* __restrict__ dst, int64_t ld) {
  const int64_t r = (int64_t)blockIdx.x * kJBS + threadIdx.x;
  const int64_t left = *d_count - list_begin;
  if (r >= (left < max_rows ? left : max_rows)) return;
  const int64_t row = rows[list_begin + r];
  if (row < 0 || row >= ld) return;
  dst[row] = src[r];
}

// byte offsets of a call's scratch
struct LieTreeLayout {
  int64_t n_blocks;
  int64_t u0, u, s, partial, ctl, mask, total;
};

inline LieTreeLayout lie_tree_layout(int64_t n_rows, int64_t G) {
  LieTreeLayout p;
  p.n_blocks = (n_rows + kJBS - 1) / kJBS;
  p.u0 = 0;
  p.u = p.u0 + 8 * G * n_rows;
  p.s = p.u + 8 * G * n_rows;
  p.partial = p.s + 8 * n_rows;
  p.ctl = p.partial + (int64_t)sizeof(LieBest) * p.n_blocks;
  p.mask = p.ctl + (int64_t)sizeof(LieCtl);
  p.total = (p.mask + n_rows + 15) & ~(int64_t)15;
  return p;
}

inline bool lie_tree_rows_ok(int64_t n_rows) {
  return n_rows >= 0 && n_rows <= (int64_t)2147483647 * kJBS && n_rows < ((int64_t)1 << 40);
}
}  // namespace
}  // namespace tpe

using namespace tpe;

extern "C" int64_t tpe_joint_lie_tree_scratch_bytes(int64_t n_rows, int n_groups) {
  if (!lie_tree_rows_ok(n_rows) || n_groups < 1 || n_groups > kJMaxD) return -1;
  return lie_tree_layout(n_rows, n_groups).total;
}

extern "C" int tpe_joint_lie_tree_picks(
    const tpe_joint_label* host_labels, const tpe_joint_label* labels, int n_labels,
    const double* tables, int64_t n_tables, const int32_t* group_off, const double* group_log_w,
    const int32_t* group_col, int n_groups, const double* sigma, const double* vals,
    const uint8_t* active, int64_t ld, int n_cols, int64_t n_rows, const double* S0,
    const double* A, int64_t ldA, double log_lie, const uint8_t* taken, const uint8_t* distinct,
    int64_t k, int64_t* out_rows, int64_t* out_count, double* S_at_pick, double* S_k,
    void* scratch, void* stream) {
  const char* fn = "tpe_joint_lie_tree_picks";
  const int rc = check_joint_labels(fn, host_labels, n_labels, n_cols,
                                    n_tables < 0 ? 0 : n_tables);
  if (rc != TPE_OK) return rc;
  if (n_groups < 1 || !group_off || !group_log_w || !group_col) {
    set_error("%s: n_groups=%d / null group arrays", fn, n_groups);
    return TPE_E_ARG;
  }
  if (n_groups > kJMaxD) {
    set_error("%s: %d groups, at most %d", fn, n_groups, kJMaxD);
    return TPE_E_UNSUPPORTED;
  }
  LieGroups grp;
  grp.n = n_groups;
  bool bad = group_off[0] != 0 || group_off[n_groups] != n_labels || group_col[0] != -1;
  for (int g = 0; g < n_groups && !bad; ++g) {
    bad = group_off[g + 1] <= group_off[g] || group_off[g + 1] > n_labels || group_col[g] < -1 ||
          group_col[g] >= n_cols || !(group_log_w[g] < INFINITY);
    grp.off[g] = group_off[g];
    grp.col[g] = group_col[g];
    grp.log_w[g] = group_log_w[g];
  }
  if (bad) {
    set_error("%s: the groups do not split the %d labels in order (the root first, its column "
              "-1), or a column is outside [0, %d), or a log W is not < inf", fn, n_labels,
              n_cols);
    return TPE_E_ARG;
  }
  grp.off[n_groups] = n_labels;
  if (!lie_tree_rows_ok(n_rows) || ld < 0 || n_rows > ld || ldA < n_rows) {
    set_error("%s: n_rows=%lld of ld=%lld, ldA=%lld", fn, (long long)n_rows, (long long)ld,
              (long long)ldA);
    return TPE_E_ARG;
  }
  if (!(log_lie < INFINITY) || !(log_lie > -INFINITY)) {
    set_error("%s: log(lie_weight)=%g", fn, log_lie);
    return TPE_E_ARG;
  }
  if (!out_count) {
    set_error("%s: null out_count", fn);
    return TPE_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  if (k <= 0 || n_rows == 0) {
    if (n_rows > 0 && S_k && !S0) {
      set_error("%s: null pointer", fn);
      return TPE_E_ARG;
    }
    if (hipMemsetAsync(out_count, 0, sizeof(int64_t), st) != hipSuccess ||
        (n_rows > 0 && S_k &&
         hipMemcpyAsync(S_k, S0, 8 * n_rows, hipMemcpyDeviceToDevice, st) != hipSuccess)) {
      set_error("%s: an async memset / copy failed", fn);
      return TPE_E_LAUNCH;
    }
    return TPE_OK;
  }
  bool cat = false, cont = false;
  for (int d = 0; d < n_labels; ++d) {
    cat |= host_labels[d].kind == TPE_JOINT_CAT;
    cont |= host_labels[d].kind != TPE_JOINT_CAT;
  }
  if (!labels || !vals || !S0 || !A || !taken || !out_rows || !scratch || (cat && !tables) ||
      (cont && !sigma) || (n_groups > 1 && !active)) {
    set_error("%s: null pointer", fn);
    return TPE_E_ARG;
  }
  if (k > n_rows) k = n_rows;
  const LieTreeLayout lay = lie_tree_layout(n_rows, n_groups);
  uint8_t* ws = static_cast<uint8_t*>(scratch);
  double* U0 = reinterpret_cast<double*>(ws + lay.u0);
  double* U = reinterpret_cast<double*>(ws + lay.u);
  double* Sw = reinterpret_cast<double*>(ws + lay.s);
  LieBest* partial = reinterpret_cast<LieBest*>(ws + lay.partial);
  LieCtl* ctl = reinterpret_cast<LieCtl*>(ws + lay.ctl);
  uint8_t* mask = ws + lay.mask;
  const dim3 grid((unsigned)lay.n_blocks), bs(kJBS);
  hipLaunchKernelGGL(k_lie_tree_init, grid, bs, 0, st, grp, S0, A, ldA, active, ld, taken,
                     distinct, n_rows, U0, U, Sw, mask, partial, ctl, out_count);
  for (int64_t j = 0; j < k; ++j) {
    hipLaunchKernelGGL(k_lie_final, dim3(1), bs, 0, st, partial, lay.n_blocks, j, Sw, mask, ctl,
                       out_rows, out_count, S_at_pick);
    // (the last pick's update only serves S_k)
    if (j + 1 < k || S_k)
      hipLaunchKernelGGL(k_lie_tree_update, grid, bs, 0, st, grp, labels, n_labels, tables, sigma,
                         vals, active, ld, n_rows, S0, log_lie, ctl, U0, U, Sw, mask, partial);
  }
  if (S_k && hipMemcpyAsync(S_k, Sw, 8 * n_rows, hipMemcpyDeviceToDevice, st) != hipSuccess) {
    set_error("%s: hipMemcpyAsync failed", fn);
    return TPE_E_LAUNCH;
  }
  return check_launch(fn);
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
