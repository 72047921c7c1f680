// tpe_grid_joint.hip -- the joint Parzen criterion (tpe_joint.hip) on a block
// of a grid pool (tpe_grid.hip), from per-axis factor tables.
//
// In the walk of tpe_joint_pass.hpp every joint label d adds to a_i a factor
// f_{d,i}(x_d) that depends on the label, the component and the label's value
// alone.  On a grid x_d is one of the n_d values of the label's axis, so the
// factors of a set form a table F of (sum_d n_d) x C doubles:
//
//   tpe_grid_joint_factors  F[(frow_d + v) * ldF + i - comp_begin] =
//                           f_{d,i}(axis_d[v]), one thread per (axis value,
//                           component), by the walk's own expressions
//                           (fit_coord, log_mass, normal_cdf, the explicit fma,
//                           (tx - mu) * (i == n ? prior_r : r)).
//   tpe_grid_joint_score    a_i of a row = log w_i + one F entry per joint
//                           label, added in label order: the walk's sequence of
//                           roundings.  A block is kGJTile consecutive rows x
//                           one chunk of kJChunk components.  The joint labels
//                           whose digit is the same in every row of the tile
//                           and that come before the first label whose digit
//                           changes are a prefix of that sum: thread i adds
//                           them once for component i of the chunk, into LDS
//                           (phase A).  Then thread = row: in passes of kJPer
//                           components a[k] starts from the LDS prefix (a
//                           broadcast) and takes one F entry per remaining
//                           label -- 64 contiguous bytes per thread, label and
//                           pass; a label behind the prefix whose digit does
//                           not change inside the tile reads one address for
//                           all lanes -- and the pass joins the running (m, s)
//                           by the walk's statements (phase B).  The chunk's
//                           (m, s) goes to scratch; after the set's last
//                           component window a second kernel merges a row's
//                           chunks (tpe_joint_pass.hpp's merge text).
//
// The decode is tpe_grid.hip's: quotient and remainder of the tile's first row
// once per (tile, label) in 64 bits; a row's digit then takes 32-bit
// arithmetic, the two divisions (by a stride below the tile, by a radix below
// 2 * kGJTile) as multiplications by a rounded-up reciprocal (exact for these
// ranges: the numerators stay below 2^11).  A label that only takes part in
// the decode (frow < 0) enters the strides and nothing else.
//
// A row's bits depend on the row, the set and kJChunk / kJPer alone: not on the
// tile, the row window, the component windows or block scheduling.  No atomics.
#include "tpe_joint.hpp"

namespace tpe {
namespace {
constexpr int kGJTile = kJBS;  // rows per tile: a thread owns one row
constexpr int kGJMax = 128;    // labels of a block per call (tpe_grid_fold's limit)
constexpr int kGJSmall = 2 * kGJTile;  // radices below it: remainder by reciprocal

// thread: component comp_begin + blockIdx % cpb * kJBS + threadIdx of axis value
// blockIdx / cpb of label d
__global__ __launch_bounds__(kJBS) void k_grid_joint_factors(
    const tpe_joint_label* __restrict__ labels, int n_labels, int d,
    const double* __restrict__ tables, const double* __restrict__ set, int64_t n,
    const double* __restrict__ axis, int64_t frow, double* __restrict__ F, int64_t ldF,
    int64_t comp_begin, int cpb) {
  const int64_t C = n + 1;
  const double* __restrict__ sig = set + C;
  const JComp* __restrict__ comp = reinterpret_cast<const JComp*>(set + set_comp_off(n_labels, C));
  const int64_t v = blockIdx.x / cpb;
  const int64_t col = (int64_t)(blockIdx.x % cpb) * kJBS + threadIdx.x;
  const int64_t i = comp_begin + col;
  double* __restrict__ dst = F + (frow + v) * ldF + col;
  if (i >= C) {  // (a place past the last component: never added to a live a_i)
    *dst = 0.0;
    return;
  }
  const tpe_joint_label lab = labels[d];
  const double x = axis[v];
  const JComp t = comp[(int64_t)d * C + i];
  const bool prior = i == n;
  double f;
  if (lab.kind == TPE_JOINT_CONT) {
    const double tx = fit_coord(x, (lab.flags & TPE_JOINT_LOG) != 0);
    const double rt = sig[n_labels + d], rp = lab.prior_r;
    const double u = (tx - t.mu) * (prior ? rp : rt);
    f = fma(-u, u, t.cst);
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
    const double sigma = sig[d];
    const double sg = prior ? lab.prior_sigma : sigma;
    f = log_mass(tu, tl, t.mu, sg) + t.cst;
  } else {
    const int64_t c = llrint(x);
    const bool in = c >= 0 && c < lab.n_cat;  // (a validated axis: always)
    const double* __restrict__ tab = tables + lab.tab_off + (in ? c : 0);
    const double hit = in ? tab[0] : kNegInf, miss = in ? tab[lab.n_cat] : kNegInf;
    const double lp = in ? tab[2 * (int64_t)lab.n_cat] : kNegInf;
    const double xc = (double)c;
    f = prior ? lp : (t.mu == xc ? hit : miss);
  }
  *dst = f;
}

struct GJArgs {  // the block's joint labels, in label order
  int64_t stride[kGJMax];  // the product of the radices of the block's later labels
  int32_t radix[kGJMax];   // >= 1
  int32_t frow[kGJMax];    // the F row of digit 0
  int n;
};

// a row's digit of a label: x = kind ? ((b + j) * ma) >> 32 : (j >= a);
// y = d0 + x; digit = r < kGJSmall ? y - ((y * mr) >> 32) * r : (y >= r ? y - r : y)
// chg: the digit changes inside the tile (else it is d0 in every row)
struct GJLab {
  int32_t frow, a, b, kind, d0, r, chg, pad_;
  uint64_t ma, mr;  // ceil(2^32 / stride), ceil(2^32 / radix)
};

__device__ __forceinline__ int32_t gj_digit(int32_t j, int32_t a, int32_t b, int32_t kind,
                                            int32_t d0, int32_t r, uint64_t ma, uint64_t mr) {
  const uint32_t x = kind ? (uint32_t)(((uint64_t)(uint32_t)(b + j) * ma) >> 32)
                          : (j >= a ? 1u : 0u);
  const uint32_t y = (uint32_t)d0 + x;
  if (r < kGJSmall) return (int32_t)(y - (uint32_t)(((uint64_t)y * mr) >> 32) * (uint32_t)r);
  return (int32_t)(y >= (uint32_t)r ? y - (uint32_t)r : y);
}

__global__ __launch_bounds__(kJBS) void k_grid_joint_score(
    const double* __restrict__ F, int64_t ldF, int64_t comp_begin,
    const double* __restrict__ logw, int64_t n, GJArgs A, int64_t row_begin, int64_t n_rows,
    double2* __restrict__ partial) {
  __shared__ double sPre[kJChunk];
  __shared__ GJLab sL[kGJMax];
  __shared__ int32_t sChg[kGJMax];
  __shared__ int32_t sFirst;  // the first label whose digit changes inside the tile
  const int64_t C = n + 1;
  const int nj = A.n;
  const int64_t t0 = (int64_t)blockIdx.x * kGJTile;  // first row of the tile in the window
  const int nv = (int)(n_rows - t0 < kGJTile ? n_rows - t0 : kGJTile);
  const int64_t first = row_begin + t0, last = first + nv - 1;
  const int64_t col0 = (int64_t)blockIdx.y * kJChunk;  // the chunk's first column of F
  const int64_t i_first = comp_begin + col0;
  for (int i = threadIdx.x; i < nj; i += kJBS) {
    const int64_t r = A.radix[i], s = A.stride[i];
    GJLab p{A.frow[i], kGJTile, 0, 0, 0, 1, 0, 0, 0, (uint64_t)1 << 32};
    int chg = 0;
    if (r > 1) {
      const int64_t q0 = first / s, q1 = last / s, rem = first - q0 * s;
      chg = q1 != q0;
      p.d0 = (int32_t)(q0 % r);
      p.r = (int32_t)r;
      p.mr = (((uint64_t)1 << 32) + (uint64_t)r - 1) / (uint64_t)r;
      if (s < kGJTile) {
        p.kind = 1;
        p.b = (int32_t)rem;
        p.ma = (((uint64_t)1 << 32) + (uint64_t)s - 1) / (uint64_t)s;
      } else {
        p.a = s - rem < kGJTile ? (int32_t)(s - rem) : kGJTile;
      }
    }
    p.chg = chg;
    sL[i] = p;
    sChg[i] = chg;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int p = 0;
    while (p < nj && !sChg[p]) ++p;
    sFirst = p;
  }
  __syncthreads();
  const int n_pre = sFirst;
  {  // phase A: thread = component; log w and the prefix's factors
    const int64_t i = i_first + threadIdx.x;
    double acc = i < C ? logw[i] : kNegInf;
    for (int d = 0; d < n_pre; ++d)
      acc = acc + F[(int64_t)(sL[d].frow + sL[d].d0) * ldF + col0 + threadIdx.x];
    sPre[threadIdx.x] = acc;
  }
  __syncthreads();
  // phase B: thread = row
  const int32_t j = (int)threadIdx.x < nv ? (int32_t)threadIdx.x : nv - 1;
  double m = kNegInf, s = 0.0;
  for (int64_t i0 = i_first; i0 < i_first + kJChunk && i0 < C; i0 += kJPer) {
    double a[kJPer];
#pragma unroll
    for (int k = 0; k < kJPer; ++k) a[k] = sPre[(int)(i0 - i_first) + k];
    for (int d = n_pre; d < nj; ++d) {
      const GJLab p = sL[d];
      const int32_t pf = __builtin_amdgcn_readfirstlane(p.frow);
      const int32_t pd = __builtin_amdgcn_readfirstlane(p.d0);
      if (!__builtin_amdgcn_readfirstlane(p.chg)) {
        // one digit for the whole tile (a radix-1 label, or a slow one, behind
        // the first fast label): a uniform address, the same adds
        const double* __restrict__ f = F + (int64_t)(pf + pd) * ldF + (i0 - comp_begin);
#pragma unroll
        for (int k = 0; k < kJPer; ++k) a[k] = a[k] + f[k];
        continue;
      }
      const int32_t pa = __builtin_amdgcn_readfirstlane(p.a);
      const int32_t pb = __builtin_amdgcn_readfirstlane(p.b);
      const int32_t pk = __builtin_amdgcn_readfirstlane(p.kind);
      const int32_t pr = __builtin_amdgcn_readfirstlane(p.r);
      const int32_t digit = gj_digit(j, pa, pb, pk, pd, pr, p.ma, p.mr);
      const double2* __restrict__ f = reinterpret_cast<const double2*>(
          F + (int64_t)(pf + digit) * ldF + (i0 - comp_begin));
#pragma unroll
      for (int k = 0; k < kJPer; k += 2) {
        const double2 v = f[k / 2];
        a[k] = a[k] + v.x;
        a[k + 1] = a[k + 1] + v.y;
      }
    }
    // (from here on: the walk's statements, tpe_joint_pass.hpp)
    // a place past the last component holds no component
#pragma unroll
    for (int k = 0; k < kJPer; ++k)
      if (i0 + k >= C) a[k] = kNegInf;
    // the pass joins the running (m, s), in component order
    double pm = a[0];
#pragma unroll
    for (int k = 1; k < kJPer; ++k) pm = a[k] > pm ? a[k] : pm;
    if (pm > m) {
      s = s * exp(m - pm);  // (m = -inf: s is 0 and stays 0)
      m = pm;
    }
#pragma unroll 1  // (rolled: one exp body, a[] rotates)
    for (int k = 0; k < kJPer; ++k) {
      const double head = a[0];
      s = s + (head == kNegInf ? 0.0 : exp(head - m));
#pragma unroll
      for (int jj = 0; jj + 1 < kJPer; ++jj) a[jj] = a[jj + 1];
      a[kJPer - 1] = head;
    }
  }
  if ((int)threadIdx.x < nv)
    partial[(i_first / kJChunk) * n_rows + t0 + threadIdx.x] = double2{m, s};
}

// out[r] = v - sub[r], or out[r] + (v - sub[r]); v = log L from the row's
// partials in chunk order
__global__ __launch_bounds__(kJBS) void k_grid_joint_merge(const double2* __restrict__ partial,
                                                           int64_t n_chunks, int64_t n_rows,
                                                           const double* __restrict__ sub,
                                                           double* __restrict__ out, int add) {
  const int64_t r = (int64_t)blockIdx.x * kJBS + threadIdx.x;
  if (r >= n_rows) return;
#define TPE_JOINT_PASS_MERGE
#include "tpe_joint_pass.hpp"
  if (sub) v = v - sub[r];
  out[r] = add ? out[r] + v : v;
}

inline int64_t gj_chunks(int64_t n) { return (n + 1 + kJChunk - 1) / kJChunk; }

// TPE_OK, or the error set: a component window of whole chunks inside ldF that
// begins at a component of the set
int check_window(const char* fn, int64_t n, int64_t ldF, int64_t comp_begin, int64_t n_comp) {
  if (n < 0 || n >= ((int64_t)1 << 40) || comp_begin < 0 || n_comp <= 0 ||
      comp_begin % kJChunk != 0 || n_comp % kJChunk != 0 || comp_begin > n || ldF < n_comp ||
      ldF % 2 != 0) {
    set_error("%s: n=%lld, components [%lld, +%lld) of ldF=%lld (whole chunks of %d)", fn,
              (long long)n, (long long)comp_begin, (long long)n_comp, (long long)ldF, kJChunk);
    return TPE_E_ARG;
  }
  return TPE_OK;
}
}  // namespace
}  // namespace tpe

using namespace tpe;

extern "C" int tpe_grid_joint_layout(int64_t* out, int n) {
  const int64_t v[4] = {kGJTile, kJChunk, kJPer, kGJMax};
  const int m = n < 4 ? (n < 0 ? 0 : n) : 4;
  for (int i = 0; i < m && out; ++i) out[i] = v[i];
  return m;
}

extern "C" int64_t tpe_grid_joint_scratch_bytes(int64_t n_rows, int64_t n) {
  if (n_rows < 0 || n < 0 || n >= ((int64_t)1 << 40)) return -1;
  return (int64_t)sizeof(double2) * n_rows * gj_chunks(n);
}

extern "C" int tpe_grid_joint_factors(const tpe_joint_label* host_labels,
                                      const tpe_joint_label* labels, int n_labels,
                                      const double* tables, int64_t n_tables, const double* set,
                                      int64_t n, const double* axes, int64_t n_axes,
                                      const int64_t* host_axis_off, const int64_t* host_axis_len,
                                      const int64_t* host_frow, double* F, int64_t ldF,
                                      int64_t n_frows, int64_t comp_begin, int64_t n_comp,
                                      void* stream) {
  int rc = check_joint_labels("tpe_grid_joint_factors", host_labels, n_labels, INT32_MAX,
                              n_tables < 0 ? 0 : n_tables);
  if (rc != TPE_OK) return rc;
  rc = check_window("tpe_grid_joint_factors", n, ldF, comp_begin, n_comp);
  if (rc != TPE_OK) return rc;
  if (!host_axis_off || !host_axis_len || !host_frow) {
    set_error("tpe_grid_joint_factors: null pointer (host arrays)");
    return TPE_E_ARG;
  }
  const int64_t cpb = n_comp / kJChunk;
  bool cat = false;
  for (int d = 0; d < n_labels; ++d) {
    cat |= host_labels[d].kind == TPE_JOINT_CAT;
    const int64_t o = host_axis_off[d], len = host_axis_len[d], fr = host_frow[d];
    if (o < 0 || len < 0 || n_axes < 0 || o > n_axes || len > n_axes - o || fr < 0 ||
        n_frows < 0 || fr > n_frows || len > n_frows - fr || len * cpb > 2147483647) {
      set_error("tpe_grid_joint_factors: label %d: axis [%lld, +%lld) of %lld, F rows from %lld "
                "of %lld", d, (long long)o, (long long)len, (long long)n_axes, (long long)fr,
                (long long)n_frows);
      return TPE_E_ARG;
    }
  }
  if (!labels || !set || !axes || !F || (cat && !tables)) {
    set_error("tpe_grid_joint_factors: null pointer");
    return TPE_E_ARG;
  }
  for (int d = 0; d < n_labels; ++d) {
    if (host_axis_len[d] == 0) continue;
    hipLaunchKernelGGL(k_grid_joint_factors, dim3((unsigned)(host_axis_len[d] * cpb)), dim3(kJBS),
                       0, (hipStream_t)stream, labels, n_labels, d, tables, set, n,
                       axes + host_axis_off[d], host_frow[d], F, ldF, comp_begin, (int)cpb);
  }
  return check_launch("tpe_grid_joint_factors");
}

extern "C" int tpe_grid_joint_score(const double* F, int64_t ldF, int64_t n_frows,
                                    int64_t comp_begin, int64_t n_comp, const double* set,
                                    int64_t n, const int64_t* host_radix,
                                    const int64_t* host_frow, int n_labels, int64_t row_begin,
                                    int64_t n_rows, const double* sub, double* out, int out_mode,
                                    void* scratch, int last, void* stream) {
  if (n_labels <= 0 || !host_radix || !host_frow) {
    set_error("tpe_grid_joint_score: n_labels=%d / null host arrays", n_labels);
    return TPE_E_ARG;
  }
  if (n_labels > kGJMax) {
    set_error("tpe_grid_joint_score: %d labels, at most %d", n_labels, kGJMax);
    return TPE_E_UNSUPPORTED;
  }
  const int rc = check_window("tpe_grid_joint_score", n, ldF, comp_begin, n_comp);
  if (rc != TPE_OK) return rc;
  const bool ends = comp_begin + n_comp > n;  // (the window holds component n, the prior)
  if ((last != 0) != ends || (out_mode != TPE_GRID_JOINT_STORE && out_mode != TPE_GRID_JOINT_ADD)) {
    set_error("tpe_grid_joint_score: last=%d but the window %s the set's last component; "
              "out_mode=%d", last, ends ? "holds" : "does not hold", out_mode);
    return TPE_E_ARG;
  }
  GJArgs A;
  A.n = 0;
  int64_t rows = 1;  // of the block
  for (int i = n_labels - 1; i >= 0; --i) {
    const int64_t r = host_radix[i], fr = host_frow[i];
    if (r < 1 || rows > INT64_MAX / r) {
      set_error("tpe_grid_joint_score: label %d: radix %lld (< 1, or the block's rows overflow)",
                i, (long long)r);
      return TPE_E_ARG;
    }
    if (fr >= 0) {
      if (n_frows < 0 || fr > n_frows || r > n_frows - fr || n_frows > INT32_MAX) {
        set_error("tpe_grid_joint_score: label %d: F rows [%lld, +%lld) of %lld", i,
                  (long long)fr, (long long)r, (long long)n_frows);
        return TPE_E_ARG;
      }
      ++A.n;
    }
    rows *= r;
  }
  if (A.n == 0) {
    set_error("tpe_grid_joint_score: no joint label (every frow < 0)");
    return TPE_E_ARG;
  }
  {
    int k = A.n;
    int64_t s = 1;
    for (int i = n_labels - 1; i >= 0; --i) {
      if (host_frow[i] >= 0) {
        --k;
        A.stride[k] = s;
        A.radix[k] = (int32_t)host_radix[i];
        A.frow[k] = (int32_t)host_frow[i];
      }
      s *= host_radix[i];
    }
    for (int i = A.n; i < kGJMax; ++i) {
      A.stride[i] = 1;
      A.radix[i] = 1;
      A.frow[i] = 0;
    }
  }
  if (row_begin < 0 || n_rows < 0 || row_begin > rows || n_rows > rows - row_begin) {
    set_error("tpe_grid_joint_score: rows [%lld, %lld + %lld) leave the block of %lld rows",
              (long long)row_begin, (long long)row_begin, (long long)n_rows, (long long)rows);
    return TPE_E_ARG;
  }
  if (n_rows == 0) return TPE_OK;
  if (!F || !set || !scratch || (last && !out)) {
    set_error("tpe_grid_joint_score: null pointer");
    return TPE_E_ARG;
  }
  const int64_t tiles = (n_rows + kGJTile - 1) / kGJTile, all = gj_chunks(n);
  int64_t chunks = n_comp / kJChunk;  // of this window, those that hold a component
  if (chunks > all - comp_begin / kJChunk) chunks = all - comp_begin / kJChunk;
  if (tiles > 2147483647 || chunks > 65535) {
    set_error("tpe_grid_joint_score: n_rows=%lld / n_comp=%lld do not fit a launch",
              (long long)n_rows, (long long)n_comp);
    return TPE_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  double2* partial = static_cast<double2*>(scratch);
  hipLaunchKernelGGL(k_grid_joint_score, dim3((unsigned)tiles, (unsigned)chunks), dim3(kJBS), 0, st,
                     F, ldF, comp_begin, set, n, A, row_begin, n_rows, partial);
  if (last)
    hipLaunchKernelGGL(k_grid_joint_merge, dim3((unsigned)tiles), dim3(kJBS), 0, st, partial, all,
                       n_rows, sub, out, out_mode == TPE_GRID_JOINT_ADD ? 1 : 0);
  return check_launch("tpe_grid_joint_score");
}
