// tpe_joint_lie_chain.hip -- the liar batch under joint="chain": a pick lies in
// every chain fit it is live in, in the fit's full mixture and in its context
// marginal at once (tpe.suggest_from_pool(joint="chain", batch="liar-chain");
// the model: hyperopt_amd/joint.py "Batches in a chain").
//
// Fit g covers the labels ctx(g) + g, the n_ctx context labels first.  Its term
// C_g is a difference of two log densities of one above mixture -- all factors,
// and the first n_ctx factors -- so a pending trial is one more component of
// both, and both contributions come from one walk over the fit's labels:
//
//   U_{g,0}[r] = log W_g + A_g[r]        V_{g,0}[r] = log W_g + B_g[r]  (n_ctx > 0)
//   c^ctx_{g,p}(r) = log(lie_weight) + sum over the first n_ctx labels of log k_d(r_d)
//   c_{g,p}(r)     = c^ctx_{g,p}(r) + sum over g's own labels      (g live in p and r)
//   V_{g,j}[r] = V_{g,j-1}[r] joined with c^ctx,  U_{g,j}[r] = U_{g,j-1}[r] joined with c
//   S_j[r] = S_0[r] - sum_g ((U_{g,j} - U_{g,0}) - (V_{g,j} - V_{g,0}))   in group
//            order; a fit without a context has no V term (tpe_joint_lie_tree's sum)
//
//   k_lie_chain_init    a thread per row: U_0 = U and, for a fit with a context,
//                       V_0 = V of the fits live in its row (planes of P doubles,
//                       group-major; V's planes cover the fits with a context
//                       alone), the working S and mask, the block's best free row
//   k_lie_final         tpe_joint_lie.hpp's, unchanged
//   k_lie_chain_update  256 rows per block.  Thread g stages whether fit g is
//                       live in the pick, thread d the pick's {mu, constant} pair
//                       of record d where its fit is (<= 128 x 16 B of LDS).  Then
//                       a thread per row walks the fits in order, with two
//                       running sums per fit.  A fit not live in the row is
//                       skipped; one not live in the pick (block-uniform) costs
//                       the loads of U, U_0, V, V_0 and the subtracts; one live in
//                       both walks its records once with the pairs as LDS
//                       broadcasts, snapshots c at the label boundary, joins V
//                       there, joins U at the end and stores both.  The penalties
//                       fold in group order into S_j, which joins the block's
//                       argmax.
//
// A context label is a record of every fit whose context holds it, evaluated
// with that fit's sigma: that is the model (the marginal is the fit's own
// mixture cut short), not a repeated computation.  Rows of different branches
// share a wave, so the group branch diverges: a wave executes at most the
// records of the fits live in any of its rows, <= the 128 records of the call.
// The fits' offsets, context sizes, V planes, liveness columns and log W travel
// by value in the kernel arguments (3 KiB): a group index is uniform, so they
// are scalar loads.  No floating-point atomics, a thread owns its row, every sum
// runs in a fixed order, the (key, row) minimum is exact: a row's bits depend on
// the row, the records and the pick sequence alone, not on P, the block or the
// grid.  With every n_ctx = 0 the arithmetic is tpe_joint_lie_tree.hip's,
// expression for expression: the same bits.
#include "tpe_joint_lie.hpp"

namespace tpe {
namespace {
struct LieChain {
  int n;                  // G
  int off[kJMaxD + 1];    // fit g's records: [off[g], off[g + 1]), its context's first
  int n_ctx[kJMaxD];      // how many of them are context labels (0: none, no V)
  int vpl[kJMaxD];        // fit g's plane of V_0 / V; -1 without a context
  int col[kJMaxD];        // the column whose `active` byte says g is live; -1: always
  double log_w[kJMaxD];   // log W_g
};
static_assert(sizeof(LieChain) < 4096, "the fits travel in the kernel arguments");

__device__ __forceinline__ bool chain_live(const LieChain& grp, int g,
                                           const uint8_t* __restrict__ active, int64_t ld,
                                           int64_t row) {
  const int c = grp.col[g];
  return c < 0 || active[(int64_t)c * ld + row] != 0;
}

// the "Batches" rule: the running term u first; c = -inf is the caller's to skip
__device__ __forceinline__ double lie_join(double u, double c) {
  const double m = c > u ? c : u;
  return m == kNegInf ? kNegInf : m + log(exp(u - m) + exp(c - m));
}

__global__ __launch_bounds__(kJBS) void k_lie_chain_init(
    const LieChain grp, const double* __restrict__ S0, const double* __restrict__ A, int64_t ldA,
    const double* __restrict__ B, int64_t ldB, const uint8_t* __restrict__ active, int64_t ld,
    const uint8_t* __restrict__ taken, const uint8_t* __restrict__ distinct, int64_t n_rows,
    double* __restrict__ U0, double* __restrict__ U, double* __restrict__ V0,
    double* __restrict__ V, double* __restrict__ Sw, uint8_t* __restrict__ mask,
    LieBest* __restrict__ partial, LieCtl* __restrict__ ctl, int64_t* __restrict__ out_count) {
  __shared__ LieBest sb[kJBS];
  const int64_t r = (int64_t)blockIdx.x * kJBS + threadIdx.x;
  LieBest mine{0, -1};
  if (r < n_rows) {
    for (int g = 0; g < grp.n; ++g) {
      if (!chain_live(grp, g, active, ld, r)) continue;
      const double u = grp.log_w[g] + A[(int64_t)g * ldA + r];
      U0[(int64_t)g * n_rows + r] = u;
      U[(int64_t)g * n_rows + r] = u;
      if (grp.n_ctx[g] > 0) {
        const double v = grp.log_w[g] + B[(int64_t)g * ldB + r];
        V0[(int64_t)grp.vpl[g] * n_rows + r] = v;
        V[(int64_t)grp.vpl[g] * n_rows + r] = v;
      }
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

__global__ __launch_bounds__(kJBS) void k_lie_chain_update(
    const LieChain grp, const tpe_joint_label* __restrict__ labels, int n_labels,
    const double* __restrict__ tables, const double* __restrict__ sig,
    const double* __restrict__ vals, const uint8_t* __restrict__ active, int64_t ld,
    int64_t n_rows, const double* __restrict__ S0, double log_lie,
    const LieCtl* __restrict__ ctl, const double* __restrict__ U0, double* __restrict__ U,
    const double* __restrict__ V0, double* __restrict__ V, double* __restrict__ Sw,
    const uint8_t* __restrict__ mask, LieBest* __restrict__ partial) {
  __shared__ JComp pick[kJMaxD];
  __shared__ uint8_t in_pick[kJMaxD];
  __shared__ LieBest sb[kJBS];
  const int64_t p = ctl->cur;
  if (p < 0) return;  // (the whole grid: no pick, nothing to add)
  for (int g = threadIdx.x; g < grp.n; g += kJBS) in_pick[g] = chain_live(grp, g, active, ld, p);
  // the pick as a trial component of each above set it is live in, context
  // records included: what k_joint_prep would write for a history row that held
  // row p (where g is live, so is all of ctx(g): the values are row p's to read)
  for (int d = threadIdx.x; d < n_labels; d += kJBS) {
    int g = 0;
    while (grp.off[g + 1] <= d) ++g;  // (off[G] = n_labels > d)
    if (!chain_live(grp, g, active, ld, p)) continue;
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
      if (!chain_live(grp, g, active, ld, r)) continue;
      const int64_t at = (int64_t)g * n_rows + r;
      const int n_ctx = grp.n_ctx[g];
      const double u = U[at];
      double un = u;
      if (n_ctx == 0) {  // tpe_joint_lie_tree.hip's group: one running sum
        if (in_pick[g]) {
          double c = log_lie;
          for (int d = grp.off[g]; d < grp.off[g + 1]; ++d) {
            const tpe_joint_label lab = labels[d];
            const double x = vals[(int64_t)lab.col * ld + r];
            c = c + lie_factor(lab, x, pick[d], sig, d, n_labels, tables);
          }
          if (c != kNegInf) {  // (c = -inf leaves U's bits)
            un = lie_join(u, c);
            U[at] = un;
          }
        }
        const double u0 = U0[at];
        if (fabs(u0) < INFINITY) s = s - (un - u0);
        continue;
      }
      const int64_t vat = (int64_t)grp.vpl[g] * n_rows + r;
      const double v = V[vat];
      double vn = v;
      if (in_pick[g]) {
        const int d0 = grp.off[g], d_own = d0 + n_ctx, d1 = grp.off[g + 1];
        double c = log_lie;
        for (int d = d0; d < d_own; ++d) {
          const tpe_joint_label lab = labels[d];
          const double x = vals[(int64_t)lab.col * ld + r];
          c = c + lie_factor(lab, x, pick[d], sig, d, n_labels, tables);
        }
        // the label boundary: c is c^ctx, and the walk goes on from it
        if (c != kNegInf) {
          vn = lie_join(v, c);
          V[vat] = vn;
          for (int d = d_own; d < d1; ++d) {
            const tpe_joint_label lab = labels[d];
            const double x = vals[(int64_t)lab.col * ld + r];
            c = c + lie_factor(lab, x, pick[d], sig, d, n_labels, tables);
          }
          // (c^ctx = -inf: c is -inf whatever follows, NaN never -- a factor is < +inf)
          if (c != kNegInf) {
            un = lie_join(u, c);
            U[at] = un;
          }
        }
      }
      const double u0 = U0[at], v0 = V0[vat];
      if (fabs(u0) < INFINITY && fabs(v0) < INFINITY) s = s - ((un - u0) - (vn - v0));
    }
    Sw[r] = s;
    if (!mask[r]) mine = LieBest{lie_key(s), r};
  }
  const LieBest best = lie_block_best(mine, sb);
  if (threadIdx.x == 0) partial[blockIdx.x] = best;
}

// byte offsets of a call's scratch; n_v: the fits with a context
struct LieChainLayout {
  int64_t n_blocks;
  int64_t u0, u, v0, v, s, partial, ctl, mask, total;
};

inline LieChainLayout lie_chain_layout(int64_t n_rows, int64_t G, int64_t n_v) {
  LieChainLayout p;
  p.n_blocks = (n_rows + kJBS - 1) / kJBS;
  p.u0 = 0;
  p.u = p.u0 + 8 * G * n_rows;
  p.v0 = p.u + 8 * G * n_rows;
  p.v = p.v0 + 8 * n_v * n_rows;
  p.s = p.v + 8 * n_v * n_rows;
  p.partial = p.s + 8 * n_rows;
  p.ctl = p.partial + (int64_t)sizeof(LieBest) * p.n_blocks;
  p.mask = p.ctl + (int64_t)sizeof(LieCtl);
  p.total = (p.mask + n_rows + 15) & ~(int64_t)15;
  return p;
}

inline bool lie_chain_rows_ok(int64_t n_rows) {
  return n_rows >= 0 && n_rows <= (int64_t)2147483647 * kJBS && n_rows < ((int64_t)1 << 40);
}
}  // namespace
}  // namespace tpe

using namespace tpe;

extern "C" int64_t tpe_joint_lie_chain_scratch_bytes(int64_t n_rows, int n_groups, int n_with_ctx) {
  if (!lie_chain_rows_ok(n_rows) || n_groups < 1 || n_groups > kJMaxD || n_with_ctx < 0 ||
      n_with_ctx >= n_groups)
    return -1;
  return lie_chain_layout(n_rows, n_groups, n_with_ctx).total;
}

extern "C" int tpe_joint_lie_chain_picks(
    const tpe_joint_label* host_labels, const tpe_joint_label* labels, int n_labels,
    const double* tables, int64_t n_tables, const int32_t* group_off, const double* group_log_w,
    const int32_t* group_col, const int32_t* group_n_ctx, int n_groups, const double* sigma,
    const double* vals, const uint8_t* active, int64_t ld, int n_cols, int64_t n_rows,
    const double* S0, const double* A, int64_t ldA, const double* B, int64_t ldB, double log_lie,
    const uint8_t* taken, const uint8_t* distinct, int64_t k, int64_t* out_rows,
    int64_t* out_count, double* S_at_pick, double* S_k, void* scratch, void* stream) {
  const char* fn = "tpe_joint_lie_chain_picks";
  // (past TPE_COND_MAX_LABELS records, contexts included: TPE_E_UNSUPPORTED)
  const int rc = check_joint_labels(fn, host_labels, n_labels, n_cols,
                                    n_tables < 0 ? 0 : n_tables);
  if (rc != TPE_OK) return rc;
  if (n_groups < 1 || !group_off || !group_log_w || !group_col || !group_n_ctx) {
    set_error("%s: n_groups=%d / null group arrays", fn, n_groups);
    return TPE_E_ARG;
  }
  if (n_groups > kJMaxD) {
    set_error("%s: %d groups, at most %d", fn, n_groups, kJMaxD);
    return TPE_E_UNSUPPORTED;
  }
  LieChain grp;
  grp.n = n_groups;
  int n_v = 0;
  bool bad = group_off[0] != 0 || group_off[n_groups] != n_labels || group_col[0] != -1 ||
             group_n_ctx[0] != 0;
  for (int g = 0; g < n_groups && !bad; ++g) {
    // (a fit has at least one label of its own after its context; one with a
    // context names its liveness column: "always live" would let the staging
    // read context values of a row in which they are not stored)
    bad = group_off[g + 1] <= group_off[g] || group_off[g + 1] > n_labels || group_col[g] < -1 ||
          group_col[g] >= n_cols || !(group_log_w[g] < INFINITY) || group_n_ctx[g] < 0 ||
          group_n_ctx[g] >= group_off[g + 1] - group_off[g] ||
          (group_n_ctx[g] > 0 && group_col[g] < 0);
    grp.off[g] = group_off[g];
    grp.col[g] = group_col[g];
    grp.log_w[g] = group_log_w[g];
    grp.n_ctx[g] = group_n_ctx[g];
    grp.vpl[g] = group_n_ctx[g] > 0 ? n_v++ : -1;
  }
  if (bad) {
    set_error("%s: the groups do not split the %d records in order (the root first, its column "
              "-1 and no context), or a column is outside [0, %d), or a context is not shorter "
              "than its fit's records or its fit has column -1, or a log W is not < inf", fn, n_labels, n_cols);
    return TPE_E_ARG;
  }
  grp.off[n_groups] = n_labels;
  if (!lie_chain_rows_ok(n_rows) || ld < 0 || n_rows > ld || ldA < n_rows ||
      (n_v > 0 && ldB < n_rows)) {
    set_error("%s: n_rows=%lld of ld=%lld, ldA=%lld, ldB=%lld", fn, (long long)n_rows,
              (long long)ld, (long long)ldA, (long long)ldB);
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
  if (!labels || !vals || !S0 || !A || (n_v > 0 && !B) || !taken || !out_rows || !scratch ||
      (cat && !tables) || (cont && !sigma) || (n_groups > 1 && !active)) {
    set_error("%s: null pointer", fn);
    return TPE_E_ARG;
  }
  if (k > n_rows) k = n_rows;
  const LieChainLayout lay = lie_chain_layout(n_rows, n_groups, n_v);
  uint8_t* ws = static_cast<uint8_t*>(scratch);
  double* U0 = reinterpret_cast<double*>(ws + lay.u0);
  double* U = reinterpret_cast<double*>(ws + lay.u);
  double* V0 = reinterpret_cast<double*>(ws + lay.v0);
  double* V = reinterpret_cast<double*>(ws + lay.v);
  double* Sw = reinterpret_cast<double*>(ws + lay.s);
  LieBest* partial = reinterpret_cast<LieBest*>(ws + lay.partial);
  LieCtl* ctl = reinterpret_cast<LieCtl*>(ws + lay.ctl);
  uint8_t* mask = ws + lay.mask;
  const dim3 grid((unsigned)lay.n_blocks), bs(kJBS);
  hipLaunchKernelGGL(k_lie_chain_init, grid, bs, 0, st, grp, S0, A, ldA, B, ldB, active, ld, taken,
                     distinct, n_rows, U0, U, V0, V, Sw, mask, partial, ctl, out_count);
  for (int64_t j = 0; j < k; ++j) {
    hipLaunchKernelGGL(k_lie_final, dim3(1), bs, 0, st, partial, lay.n_blocks, j, Sw, mask, ctl,
                       out_rows, out_count, S_at_pick);
    // (the last pick's update only serves S_k)
    if (j + 1 < k || S_k)
      hipLaunchKernelGGL(k_lie_chain_update, grid, bs, 0, st, grp, labels, n_labels, tables, sigma,
                         vals, active, ld, n_rows, S0, log_lie, ctl, U0, U, V0, V, Sw, mask,
                         partial);
  }
  if (S_k && hipMemcpyAsync(S_k, Sw, 8 * n_rows, hipMemcpyDeviceToDevice, st) != hipSuccess) {
    set_error("%s: hipMemcpyAsync failed", fn);
    return TPE_E_LAUNCH;
  }
  return check_launch(fn);
}
