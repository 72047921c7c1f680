// tpe_joint_lie.hip -- a batch of pool rows picked one at a time, each pick
// entering the above mixture as the pending trial it is about to become
// (tpe.suggest_from_pool(joint=True, batch="liar"); the model:
// hyperopt_amd/joint.py "Batches").
//
// L_above is a sum of product kernels, so a pick p joins it as one more
// component: for every pool row r
//
//   c_p(r) = log(lie_weight) + sum_d log k_d(r_d)      (d in list order)
//   U_j[r] = m + log(exp(U_{j-1}[r] - m) + exp(c_p(r) - m)),  m = max(U_{j-1}[r], c_p(r))
//   S_j[r] = S_0[r] - (U_j[r] - U_0[r])   where U_0[r] = log W + A_0[r] is finite
//
// with k_d the factor of a trial component of the above set whose observation
// is row p's stored value (tpe_joint.hip's k_joint_prep and the walk of
// tpe_joint_pass.hpp, for one component).  O(P D) per pick.
//
//   k_lie_init    U_0, the working copies of S and of the mask, and every
//                 block's best untaken row of S_0
//   k_lie_final   one block: the best of the blocks' bests is pick j -- its row
//                 to out_rows[j] and to the control word the next update reads,
//                 its byte of the working mask set
//   k_lie_update  the first D threads of each block build the pick's {mu,
//                 constant} pairs in LDS; a thread per row adds the factors,
//                 updates U, writes S_j and the block's best untaken row
//
// All k picks are enqueued at once: a pick's row index is read on the device.
// The order is tpe_pool_topk's: ascending (pool key, row) -- larger S first,
// NaN before everything, equal scores to the smaller row.  The minimum of such
// pairs is exact in any order, a thread owns its row alone, there are no
// atomics: a row's bits depend on the row, the set and the pick sequence only.
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

__global__ __launch_bounds__(kJBS) void k_lie_init(const double* __restrict__ S0,
                                                   const double* __restrict__ A0, double log_w,
                                                   const uint8_t* __restrict__ taken,
                                                   const uint8_t* __restrict__ distinct,
                                                   int64_t n_rows, double* __restrict__ U0,
                                                   double* __restrict__ U, double* __restrict__ Sw,
                                                   uint8_t* __restrict__ mask,
                                                   LieBest* __restrict__ partial,
                                                   LieCtl* __restrict__ ctl,
                                                   int64_t* __restrict__ out_count) {
  __shared__ LieBest sb[kJBS];
  const int64_t r = (int64_t)blockIdx.x * kJBS + threadIdx.x;
  LieBest mine{0, -1};
  if (r < n_rows) {
    const double u = log_w + A0[r], s = S0[r];
    const uint8_t gone = (taken[r] != 0) | (distinct ? distinct[r] != 0 : 0);
    U0[r] = u;
    U[r] = u;
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

__global__ __launch_bounds__(kJBS) void k_lie_update(const tpe_joint_label* __restrict__ labels,
                                                     int n_labels,
                                                     const double* __restrict__ tables,
                                                     const double* __restrict__ sig,
                                                     const double* __restrict__ vals, int64_t ld,
                                                     int64_t n_rows,
                                                     const double* __restrict__ S0,
                                                     double log_lie,
                                                     const LieCtl* __restrict__ ctl,
                                                     const double* __restrict__ U0,
                                                     double* __restrict__ U,
                                                     double* __restrict__ Sw,
                                                     const uint8_t* __restrict__ mask,
                                                     LieBest* __restrict__ partial) {
  __shared__ JComp pick[kJMaxD];
  __shared__ LieBest sb[kJBS];
  const int64_t p = ctl->cur;
  if (p < 0) return;  // (the whole grid: no pick, nothing to add)
  // the pick as a trial component of the above set: what k_joint_prep would
  // write for a history row that held row p (a pool's values carry no shift)
  for (int d = threadIdx.x; d < n_labels; d += kJBS) {
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
    double c = log_lie;
    for (int d = 0; d < n_labels; ++d) {
      const tpe_joint_label lab = labels[d];
      const double x = vals[(int64_t)lab.col * ld + r];
      const JComp t = pick[d];
      if (lab.kind == TPE_JOINT_CONT) {
        const double tx = fit_coord(x, (lab.flags & TPE_JOINT_LOG) != 0);
        const double u = (tx - t.mu) * sig[n_labels + d];
        c = c + fma(-u, u, t.cst);
      } else if (lab.kind == TPE_JOINT_QUANT) {
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
        c = c + (log_mass(tu, tl, t.mu, sig[d]) + t.cst);
      } else {
        const int64_t q = llrint(x);
        const bool in = q >= 0 && q < lab.n_cat;  // (a validated pool: always)
        const double* __restrict__ tab = tables + lab.tab_off + (in ? q : 0);
        const double hit = in ? tab[0] : kNegInf, miss = in ? tab[lab.n_cat] : kNegInf;
        c = c + (t.mu == (double)q ? hit : miss);
      }
    }
    const double u = U[r];
    double un = u;
    if (c != kNegInf) {  // (c = -inf leaves U's bits)
      const double m = c > u ? c : u;
      un = m == kNegInf ? kNegInf : m + log(exp(u - m) + exp(c - m));
      U[r] = un;
    }
    const double u0 = U0[r], s0 = S0[r];
    const double s = fabs(u0) < INFINITY ? s0 - (un - u0) : s0;
    Sw[r] = s;
    if (!mask[r]) mine = LieBest{lie_key(s), r};
  }
  const LieBest best = lie_block_best(mine, sb);
  if (threadIdx.x == 0) partial[blockIdx.x] = best;
}

// byte offsets of a call's scratch
struct LieLayout {
  int64_t n_blocks;
  int64_t u0, u, s, partial, ctl, mask, total;
};

inline LieLayout lie_layout(int64_t n_rows) {
  LieLayout p;
  p.n_blocks = (n_rows + kJBS - 1) / kJBS;
  p.u0 = 0;
  p.u = p.u0 + 8 * n_rows;
  p.s = p.u + 8 * n_rows;
  p.partial = p.s + 8 * n_rows;
  p.ctl = p.partial + (int64_t)sizeof(LieBest) * p.n_blocks;
  p.mask = p.ctl + (int64_t)sizeof(LieCtl);
  p.total = (p.mask + n_rows + 15) & ~(int64_t)15;
  return p;
}
static_assert(sizeof(LieBest) == 16 && sizeof(LieCtl) == 16, "the scratch stays 16-byte aligned");
}  // namespace
}  // namespace tpe

using namespace tpe;

extern "C" int64_t tpe_joint_lie_scratch_bytes(int64_t n_rows) {
  if (n_rows < 0 || n_rows > (int64_t)2147483647 * kJBS) return -1;
  return lie_layout(n_rows).total;
}

extern "C" int tpe_joint_lie_picks(const tpe_joint_label* host_labels,
                                   const tpe_joint_label* labels, int n_labels,
                                   const double* tables, int64_t n_tables, const double* sigma,
                                   const double* vals, int64_t ld, int n_cols, int64_t n_rows,
                                   const double* S0, const double* A0, double log_w,
                                   double log_lie, const uint8_t* taken, const uint8_t* distinct,
                                   int64_t k, int64_t* out_rows, int64_t* out_count,
                                   double* S_at_pick, double* S_k, void* scratch, void* stream) {
  const int rc = check_joint_labels("tpe_joint_lie_picks", host_labels, n_labels, n_cols,
                                    n_tables < 0 ? 0 : n_tables);
  if (rc != TPE_OK) return rc;
  if (n_rows < 0 || ld < 0 || n_rows > ld || n_rows > (int64_t)2147483647 * kJBS) {
    set_error("tpe_joint_lie_picks: n_rows=%lld of ld=%lld", (long long)n_rows, (long long)ld);
    return TPE_E_ARG;
  }
  if (!(log_w < INFINITY) || !(log_lie < INFINITY) || !(log_lie > -INFINITY)) {
    set_error("tpe_joint_lie_picks: log W=%g log(lie_weight)=%g", log_w, log_lie);
    return TPE_E_ARG;
  }
  if (!out_count) {
    set_error("tpe_joint_lie_picks: null out_count");
    return TPE_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  if (k <= 0 || n_rows == 0) {
    if (n_rows > 0 && S_k && !S0) {
      set_error("tpe_joint_lie_picks: null pointer");
      return TPE_E_ARG;
    }
    if (hipMemsetAsync(out_count, 0, sizeof(int64_t), st) != hipSuccess ||
        (n_rows > 0 && S_k &&
         hipMemcpyAsync(S_k, S0, 8 * n_rows, hipMemcpyDeviceToDevice, st) != hipSuccess)) {
      set_error("tpe_joint_lie_picks: an async memset / copy failed");
      return TPE_E_LAUNCH;
    }
    return TPE_OK;
  }
  bool cat = false, cont = false;
  for (int d = 0; d < n_labels; ++d) {
    cat |= host_labels[d].kind == TPE_JOINT_CAT;
    cont |= host_labels[d].kind != TPE_JOINT_CAT;
  }
  if (!labels || !vals || !S0 || !A0 || !taken || !out_rows || !scratch || (cat && !tables) ||
      (cont && !sigma)) {
    set_error("tpe_joint_lie_picks: null pointer");
    return TPE_E_ARG;
  }
  if (k > n_rows) k = n_rows;
  const LieLayout lay = lie_layout(n_rows);
  uint8_t* ws = static_cast<uint8_t*>(scratch);
  double* U0 = reinterpret_cast<double*>(ws + lay.u0);
  double* U = reinterpret_cast<double*>(ws + lay.u);
  double* Sw = reinterpret_cast<double*>(ws + lay.s);
  LieBest* partial = reinterpret_cast<LieBest*>(ws + lay.partial);
  LieCtl* ctl = reinterpret_cast<LieCtl*>(ws + lay.ctl);
  uint8_t* mask = ws + lay.mask;
  const dim3 grid((unsigned)lay.n_blocks), bs(kJBS);
  hipLaunchKernelGGL(k_lie_init, grid, bs, 0, st, S0, A0, log_w, taken, distinct, n_rows, U0, U,
                     Sw, mask, partial, ctl, out_count);
  for (int64_t j = 0; j < k; ++j) {
    hipLaunchKernelGGL(k_lie_final, dim3(1), bs, 0, st, partial, lay.n_blocks, j, Sw, mask, ctl,
                       out_rows, out_count, S_at_pick);
    // (the last pick's update only serves S_k)
    if (j + 1 < k || S_k)
      hipLaunchKernelGGL(k_lie_update, grid, bs, 0, st, labels, n_labels, tables, sigma, vals, ld,
                         n_rows, S0, log_lie, ctl, U0, U, Sw, mask, partial);
  }
  if (S_k && hipMemcpyAsync(S_k, Sw, 8 * n_rows, hipMemcpyDeviceToDevice, st) != hipSuccess) {
    set_error("tpe_joint_lie_picks: hipMemcpyAsync failed");
    return TPE_E_LAUNCH;
  }
  return check_launch("tpe_joint_lie_picks");
}
