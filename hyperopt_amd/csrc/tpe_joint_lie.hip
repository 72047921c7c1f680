// tpe_joint_lie.hip -- a batch of pool rows picked one at a time, each pick
// entering the above mixtures as the pending trial it is about to become: one
// engine behind three entries (the model: hyperopt_amd/joint.py "Batches",
// "Batches in a tree", "Batches in a chain").
//
//   tpe_joint_lie_chain_picks  joint="chain", batch="liar-chain": G fits, fit g
//                              over the labels ctx(g) + g, the n_ctx context
//                              labels first
//   tpe_joint_lie_tree_picks   joint="tree", batch="liar-tree": the chain call
//                              with every n_ctx = 0
//   tpe_joint_lie_picks        joint=True, batch="liar": the tree call with G = 1
//
// Every fit g has its own above mixture, so it keeps its own U; its term under
// "chain" is a difference of two log densities of that one mixture -- all
// factors, and the first n_ctx factors -- so a pending trial is one more
// component of both, and both contributions come from one walk over the fit's
// records:
//
//   U_{g,0}[r] = log W_g + A_g[r]        V_{g,0}[r] = log W_g + B_g[r]  (n_ctx > 0)
//   c^ctx_{g,p}(r) = log(lie_weight) + sum over the first n_ctx records of log k_d(r_d)
//   c_{g,p}(r)     = c^ctx_{g,p}(r) + sum over g's own records     (g live in p and r)
//   V_{g,j}[r] = V_{g,j-1}[r] joined with c^ctx,  U_{g,j}[r] = U_{g,j-1}[r] joined with c:
//                u joined with c = m + log(exp(u - m) + exp(c - m)),  m = max(u, c)
//   S_j[r] = S_0[r] - sum_g ((U_{g,j} - U_{g,0}) - (V_{g,j} - V_{g,0}))   in group
//            order over the fits live in r whose U_{g,0} (and V_{g,0}) is finite;
//            a fit without a context has no V term: S_j = S_{..} - (U_{g,j} - U_{g,0})
//
// with k_d the factor of a trial component of g's above set whose observation
// is row p's stored value (tpe_joint.hip's k_joint_prep and the walk of
// tpe_joint_pass.hpp, for one component).  O(P D) per pick.
//
//   k_lie_init    a thread per row: U_0 = U and, for a fit with a context, V_0 = V
//                 of the fits live in its row (planes of P doubles, group-major: a
//                 wave's accesses coalesce; V's planes cover the fits with a
//                 context alone; places of fits not live in the row are never
//                 read), the working S and mask, the block's best free row
//   k_lie_final   one block: the best of the blocks' bests is pick j -- its row
//                 to out_rows[j] and to the control word the next update reads,
//                 its byte of the working mask set
//   k_lie_update  256 rows per block.  Thread g stages whether fit g is live in
//                 the pick, thread d the pick's {mu, constant} pair of record d
//                 where its fit is (<= 128 x 16 B of LDS).  Then a thread per row
//                 walks the fits in order.  A fit not live in the row is skipped;
//                 one not live in the pick (block-uniform) costs the loads of U,
//                 U_0 (V, V_0) and the subtracts; one live in both walks its
//                 records once with the pairs as LDS broadcasts, snapshots c at
//                 the label boundary and joins V there, joins U at the end and
//                 stores both.  The penalties fold in group order into S_j, which
//                 joins the block's argmax.
//
// Both kernels are templates on kCtx.  <false> has no V planes and reads no
// n_ctx: the kernels of a flat and a tree call, and of a chain call whose
// contexts are all empty.  <true> is launched when some fit has a context.
//
// A context label is a record of every fit whose context holds it, evaluated
// with that fit's sigma: that is the model (the marginal is the fit's own
// mixture cut short), not a repeated computation.  Rows of different branches
// share a wave, so the group branch diverges: a wave executes at most the
// records of the fits live in any of its rows, <= the 128 records of the call.
// The fits' offsets, context sizes, V planes, liveness columns and log W travel
// by value in the kernel arguments (3 KiB): a group index is uniform, so they
// are scalar loads.
//
// All k picks are enqueued at once: a pick's row index is read on the device.
// The order is tpe_pool_topk's: ascending (pool key, row) -- larger S first,
// NaN before everything, equal scores to the smaller row.  The minimum of such
// pairs is exact in any order, a thread owns its row alone, every sum runs in a
// fixed order, there are no atomics: a row's bits depend on the row, the
// records and the pick sequence alone, not on P, the block, the grid or the
// entry the call came through.
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
static_assert(sizeof(LieBest) == 16 && sizeof(LieCtl) == 16, "the scratch stays 16-byte aligned");

struct LieGroups {
  int n;                  // G
  int off[kJMaxD + 1];    // fit g's records: [off[g], off[g + 1]), its context's first
  int n_ctx[kJMaxD];      // how many of them are context labels (0: none, no V)
  int vpl[kJMaxD];        // fit g's plane of V_0 / V; -1 without a context
  int col[kJMaxD];        // the column whose `active` byte says g is live; -1: always
  double log_w[kJMaxD];   // log W_g
};
static_assert(sizeof(LieGroups) < 4096, "the fits travel in the kernel arguments");

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

__device__ __forceinline__ bool lie_live(const LieGroups& grp, int g,
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

// log k_d of the stored value x under the pick's pair t: the factor
// expressions of tpe_joint_pass.hpp for one trial component.  sig is read for
// a label with a bandwidth only: it may be NULL when every label is discrete.
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

template <bool kCtx>
__global__ __launch_bounds__(kJBS) void k_lie_init(
    const LieGroups grp, const double* __restrict__ S0, const double* __restrict__ A, int64_t ldA,
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
      if (!lie_live(grp, g, active, ld, r)) continue;
      const double u = grp.log_w[g] + A[(int64_t)g * ldA + r];
      U0[(int64_t)g * n_rows + r] = u;
      U[(int64_t)g * n_rows + r] = u;
      if (kCtx && grp.n_ctx[g] > 0) {
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

template <bool kCtx>
__global__ __launch_bounds__(kJBS) void k_lie_update(
    const LieGroups grp, const tpe_joint_label* __restrict__ labels, int n_labels,
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
  for (int g = threadIdx.x; g < grp.n; g += kJBS) in_pick[g] = lie_live(grp, g, active, ld, p);
  // the pick as a trial component of each above set it is live in, context
  // records included: what k_joint_prep would write for a history row that held
  // row p (a pool's values carry no shift; where g is live, so is all of
  // ctx(g): the values are row p's to read)
  for (int d = threadIdx.x; d < n_labels; d += kJBS) {
    int g = 0;
    while (grp.off[g + 1] <= d) ++g;  // (off[G] = n_labels > d)
    if (!lie_live(grp, g, active, ld, p)) continue;  // (its values are not row p's to read)
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
    // c after the records [d0, d1) of the walk, from c
    auto walk = [&](double c, int d0, int d1) {
      for (int d = d0; d < d1; ++d) {
        const tpe_joint_label lab = labels[d];
        const double x = vals[(int64_t)lab.col * ld + r];
        c = c + lie_factor(lab, x, pick[d], sig, d, n_labels, tables);
      }
      return c;
    };
    double s = S0[r];
    for (int g = 0; g < grp.n; ++g) {
      if (!lie_live(grp, g, active, ld, r)) continue;
      const int64_t at = (int64_t)g * n_rows + r;
      const int n_ctx = kCtx ? grp.n_ctx[g] : 0;
      const int d_own = grp.off[g] + n_ctx, d1 = grp.off[g + 1];
      const double u = U[at];
      double un = u;
      if (n_ctx == 0) {  // one running sum, no V
        if (in_pick[g]) {
          const double c = walk(log_lie, d_own, d1);
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
        double c = walk(log_lie, grp.off[g], d_own);
        // the label boundary: c is c^ctx, and the walk goes on from it
        if (c != kNegInf) {
          vn = lie_join(v, c);
          V[vat] = vn;
          c = walk(c, d_own, d1);
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
struct LieLayout {
  int64_t n_blocks;
  int64_t u0, u, v0, v, s, partial, ctl, mask, total;
};

inline LieLayout lie_layout(int64_t n_rows, int64_t G, int64_t n_v) {
  LieLayout p;
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

// (a grid of at most 2^31 - 1 blocks: below 2^40 rows)
inline bool lie_rows_ok(int64_t n_rows) {
  return n_rows >= 0 && n_rows <= (int64_t)2147483647 * kJBS;
}

// The call behind the three entries, `fn` the entry's name.  B and ldB are read
// where some fit has a context.
int lie_picks(const char* fn, const tpe_joint_label* host_labels, const tpe_joint_label* labels,
              int n_labels, const double* tables, int64_t n_tables, const int32_t* group_off,
              const double* group_log_w, const int32_t* group_col, const int32_t* group_n_ctx,
              int n_groups, const double* sigma, const double* vals, const uint8_t* active,
              int64_t ld, int n_cols, int64_t n_rows, const double* S0, const double* A,
              int64_t ldA, const double* B, int64_t ldB, double log_lie, const uint8_t* taken,
              const uint8_t* distinct, int64_t k, int64_t* out_rows, int64_t* out_count,
              double* S_at_pick, double* S_k, void* scratch, void* stream) {
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
  LieGroups grp;
  grp.n = n_groups;
  int n_v = 0;
  bool bad = group_off[0] != 0 || group_off[n_groups] != n_labels || group_col[0] != -1;
  for (int g = 0; g < n_groups && !bad; ++g) {
    // (a fit has at least one label of its own after its context; one with a
    // context is not the root and names its liveness column: "always live"
    // would let the staging read context values of a row in which they are not
    // stored)
    const int n_ctx = group_n_ctx[g];
    bad = group_off[g + 1] <= group_off[g] || group_off[g + 1] > n_labels || group_col[g] < -1 ||
          group_col[g] >= n_cols || !(group_log_w[g] < INFINITY) || n_ctx < 0 ||
          n_ctx >= group_off[g + 1] - group_off[g] || (n_ctx > 0 && group_col[g] < 0);
    grp.off[g] = group_off[g];
    grp.col[g] = group_col[g];
    grp.log_w[g] = group_log_w[g];
    grp.n_ctx[g] = n_ctx;
    grp.vpl[g] = n_ctx > 0 ? n_v++ : -1;
  }
  if (bad) {
    set_error("%s: the groups do not split the %d records in order (the root first, its column "
              "-1 and no context), or a column is outside [0, %d), or a context is not shorter "
              "than its fit's records or its fit has column -1, or a log W is not < inf",
              fn, n_labels, n_cols);
    return TPE_E_ARG;
  }
  grp.off[n_groups] = n_labels;
  if (!lie_rows_ok(n_rows) || ld < 0 || n_rows > ld || ldA < n_rows ||
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
  const LieLayout lay = lie_layout(n_rows, n_groups, n_v);
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
  hipLaunchKernelGGL(n_v > 0 ? k_lie_init<true> : k_lie_init<false>, grid, bs, 0, st, grp, S0, A,
                     ldA, B, ldB, active, ld, taken, distinct, n_rows, U0, U, V0, V, Sw, mask,
                     partial, ctl, out_count);
  for (int64_t j = 0; j < k; ++j) {
    hipLaunchKernelGGL(k_lie_final, dim3(1), bs, 0, st, partial, lay.n_blocks, j, Sw, mask, ctl,
                       out_rows, out_count, S_at_pick);
    // (the last pick's update only serves S_k)
    if (j + 1 < k || S_k)
      hipLaunchKernelGGL(n_v > 0 ? k_lie_update<true> : k_lie_update<false>, grid, bs, 0, st, grp,
                         labels, n_labels, tables, sigma, vals, active, ld, n_rows, S0, log_lie,
                         ctl, U0, U, V0, V, Sw, mask, partial);
  }
  if (S_k && hipMemcpyAsync(S_k, Sw, 8 * n_rows, hipMemcpyDeviceToDevice, st) != hipSuccess) {
    set_error("%s: hipMemcpyAsync failed", fn);
    return TPE_E_LAUNCH;
  }
  return check_launch(fn);
}

const int32_t kNoCtx[kJMaxD] = {};  // group_n_ctx of a call without contexts
}  // namespace
}  // namespace tpe

using namespace tpe;

extern "C" int64_t tpe_joint_lie_chain_scratch_bytes(int64_t n_rows, int n_groups, int n_with_ctx) {
  if (!lie_rows_ok(n_rows) || n_groups < 1 || n_groups > kJMaxD || n_with_ctx < 0 ||
      n_with_ctx >= n_groups)
    return -1;
  return lie_layout(n_rows, n_groups, n_with_ctx).total;
}

extern "C" int64_t tpe_joint_lie_tree_scratch_bytes(int64_t n_rows, int n_groups) {
  return tpe_joint_lie_chain_scratch_bytes(n_rows, n_groups, 0);
}

extern "C" int64_t tpe_joint_lie_scratch_bytes(int64_t n_rows) {
  return tpe_joint_lie_chain_scratch_bytes(n_rows, 1, 0);
}

extern "C" int tpe_joint_lie_chain_picks(
    const tpe_joint_label* host_labels, const tpe_joint_label* labels, int n_labels,
    const double* tables, int64_t n_tables, const int32_t* group_off, const double* group_log_w,
    const int32_t* group_col, const int32_t* group_n_ctx, int n_groups, const double* sigma,
    const double* vals, const uint8_t* active, int64_t ld, int n_cols, int64_t n_rows,
    const double* S0, const double* A, int64_t ldA, const double* B, int64_t ldB, double log_lie,
    const uint8_t* taken, const uint8_t* distinct, int64_t k, int64_t* out_rows,
    int64_t* out_count, double* S_at_pick, double* S_k, void* scratch, void* stream) {
  return lie_picks("tpe_joint_lie_chain_picks", host_labels, labels, n_labels, tables, n_tables, group_off, group_log_w,
                   group_col, group_n_ctx, n_groups, sigma, vals, active, ld, n_cols, n_rows, S0,
                   A, ldA, B, ldB, log_lie, taken, distinct, k, out_rows, out_count, S_at_pick,
                   S_k, scratch, stream);
}

extern "C" int tpe_joint_lie_tree_picks(
    const tpe_joint_label* host_labels, const tpe_joint_label* labels, int n_labels,
    const double* tables, int64_t n_tables, const int32_t* group_off, const double* group_log_w,
    const int32_t* group_col, int n_groups, const double* sigma, const double* vals,
    const uint8_t* active, int64_t ld, int n_cols, int64_t n_rows, const double* S0,
    const double* A, int64_t ldA, double log_lie, const uint8_t* taken, const uint8_t* distinct,
    int64_t k, int64_t* out_rows, int64_t* out_count, double* S_at_pick, double* S_k,
    void* scratch, void* stream) {
  return lie_picks("tpe_joint_lie_tree_picks", host_labels, labels, n_labels, tables, n_tables,
                   group_off, group_log_w, group_col, kNoCtx, n_groups, sigma, vals, active, ld,
                   n_cols, n_rows, S0, A, ldA, nullptr, 0, log_lie, taken, distinct, k, out_rows,
                   out_count, S_at_pick, S_k, scratch, stream);
}

// one group of all the labels, always live: A = A0, a single plane
extern "C" int tpe_joint_lie_picks(const tpe_joint_label* host_labels,
                                   const tpe_joint_label* labels, int n_labels,
                                   const double* tables, int64_t n_tables, const double* sigma,
                                   const double* vals, int64_t ld, int n_cols, int64_t n_rows,
                                   const double* S0, const double* A0, double log_w,
                                   double log_lie, const uint8_t* taken, const uint8_t* distinct,
                                   int64_t k, int64_t* out_rows, int64_t* out_count,
                                   double* S_at_pick, double* S_k, void* scratch, void* stream) {
  const int32_t off[2] = {0, n_labels}, col[1] = {-1};
  return lie_picks("tpe_joint_lie_picks", host_labels, labels, n_labels, tables, n_tables, off,
                   &log_w, col, kNoCtx, 1, sigma, vals, nullptr, ld, n_cols, n_rows, S0, A0,
                   n_rows, nullptr, 0, log_lie, taken, distinct, k, out_rows, out_count, S_at_pick,
                   S_k, scratch, stream);
}
