// tpe_grid.hip -- the joint score of a Cartesian product of per-label axes
// (tpe.GridPool), folded from per-value terms without the product's rows.
//
// A block of a grid pool is the product of the axes of its live labels: row r
// of the block holds digit_i(r) of label i, the mixed-radix digits of r with
// the last label fastest (itertools.product order).  The exact scorers have
// left log l and log g of every axis value in bl / al; the criterion of
// tpe_pool.hip is separable over them,
//
//   S[r] = sum_i (bl[off_i + digit_i(r)] - al[off_i + digit_i(r)]),
//
// a sequential fp64 sum from 0.0 in label order (-ffp-contract=off): the bits
// k_pool_fold gives for the materialised row.
//
// One workgroup folds a tile of kGTile consecutive rows.  The 64-bit decode is
// done once per (tile, label): with s_i the stride of label i (the product of
// the radices after it), q0_i = first / s_i and rem_i = first % s_i for the
// tile's first row, row first + j has
//
//   row / s_i = q0_i + (rem_i + j) / s_i,      j < kGTile,
//
// so inside the tile the quotient moves by x_i(j) = (rem_i + j) / s_i: a
// 32-bit division when s_i < kGTile, and j >= s_i - rem_i (0 or 1) otherwise.
// The differences bl - al of the quotients q0_i .. q0_i + x_i(last) are staged
// in LDS once per tile, entry x at digit (q0_i + x) % radix_i, and a row reads
// entry x_i(j) of every label.  Where the tile takes every digit of a label
// the axis is staged whole instead, entry x at digit x, and a row reads entry
// (q0_i + x_i(j)) % radix_i, again in 32 bits.  No 64-bit division per row.
// Labels of radix >= 2 have strides that at least double
// from one to the next, so a tile stages fewer than 2 * kGTile + 2 * n_labels
// entries whatever the radices (kGTerms); there is no second code path for
// large axes.  Only entries of digits that rows of the window take are read.
// Thread t owns rows t, t + 256, ...: the stores to S are coalesced.
#include "tpe_common.hpp"

namespace tpe {
namespace {
constexpr int kGBS = 256;                // threads per block
constexpr int kGTile = 2048;             // rows per tile
constexpr int kGPer = kGTile / kGBS;     // rows per thread
constexpr int kGridMax = 128;            // labels per call
constexpr int kGTerms = 2 * kGTile + 2 * kGridMax;

struct GridArgs {
  int64_t off[kGridMax];    // bl / al element of the label's digit 0
  int64_t radix[kGridMax];  // >= 1
  int n;
};

// a row's entry of label i, base + x:
//   kind 0 (stride >= kGTile, or radix 1)   x = j >= a
//   kind 1 (stride a < kGTile)              x = (b + j) / a
//   kind 2 (... and the axis staged whole)  x = ((b + j) / a + c) % r
struct GridLab {
  int32_t base, a, b, kind, c, r;
};
// the staged entries of label i: entry x is digit (d0 + x) % radix
struct GridStage {
  int64_t off, radix, d0;
};

// Onto: the accumulator starts from S (tpe_grid_fold_onto), and a label with
// off < 0 takes part in the decode alone: it stages nothing and adds nothing
// (kind 3)
template <bool Onto>
__global__ __launch_bounds__(kGBS) void k_grid_fold(const double* __restrict__ bl,
                                                    const double* __restrict__ al, GridArgs A,
                                                    int64_t row_begin, int64_t n_rows,
                                                    double* __restrict__ S) {
  __shared__ double sD[kGTerms];
  __shared__ int64_t sStride[kGridMax];
  __shared__ GridStage sS[kGridMax];
  __shared__ GridLab sL[kGridMax];
  __shared__ int32_t sBase[kGridMax + 1];  // counts, then exclusive offsets and the total
  const int n = A.n;
  const int64_t t0 = (int64_t)blockIdx.x * kGTile;  // first row of the tile in the window
  const int nv = (int)(n_rows - t0 < kGTile ? n_rows - t0 : kGTile);
  const int64_t first = row_begin + t0, last = first + nv - 1;
  if (threadIdx.x == 0) {
    int64_t s = 1;
    for (int i = n - 1; i >= 0; --i) {
      sStride[i] = s;
      s *= A.radix[i];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += kGBS) {
    const int64_t r = A.radix[i], s = sStride[i];
    GridLab p{0, INT32_MAX, 0, 0, 0, 1};
    GridStage g{A.off[i], r, 0};
    int cnt = 1;
    if (r > 1) {
      const int64_t q0 = first / s, q1 = last / s, rem = first - q0 * s;
      cnt = (int)(q1 - q0 + 1);
      g.d0 = q0 % r;
      if (s < kGTile) {
        p.a = (int32_t)s;
        p.b = (int32_t)rem;
        p.kind = 1;
        if (cnt >= r) {  // every digit: entry x is digit x
          p.kind = 2;
          p.c = (int32_t)g.d0;
          p.r = (int32_t)r;
          cnt = (int)r;
          g.d0 = 0;
        }
      } else {
        p.a = s - rem < kGTile ? (int32_t)(s - rem) : kGTile;
      }
    }
    if (Onto && A.off[i] < 0) {
      p.kind = 3;
      cnt = 0;
    }
    sL[i] = p;
    sS[i] = g;
    sBase[i] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t c = 0;
    for (int i = 0; i < n; ++i) {
      const int32_t m = sBase[i];
      sBase[i] = c;
      sL[i].base = c;
      c += m;
    }
    sBase[n] = c < kGTerms ? c : kGTerms;  // (c < kGTerms by the bound above)
  }
  __syncthreads();
  const int total = sBase[n];
  for (int e = threadIdx.x; e < total; e += kGBS) {
    int lo = 0, hi = n - 1;  // the label of entry e: the last i with sBase[i] <= e
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (sBase[mid] <= e) {
        lo = mid;
      } else {
        hi = mid - 1;
      }
    }
    const GridStage g = sS[lo];
    int64_t d = g.d0 + (e - sBase[lo]);
    if (d >= g.radix)
      d = g.radix <= 0x7fffffff ? (int64_t)((uint32_t)d % (uint32_t)g.radix) : d % g.radix;
    sD[e] = bl[g.off + d] - al[g.off + d];
  }
  __syncthreads();
  double acc[kGPer];
  int32_t j[kGPer];
#pragma unroll
  for (int k = 0; k < kGPer; ++k) {
    const int row = (int)threadIdx.x + k * kGBS;
    j[k] = row < nv ? row : nv - 1;  // (a row past the tile's end reads a staged entry too)
    acc[k] = Onto ? S[t0 + j[k]] : 0.0;
  }
  for (int i = 0; i < n; ++i) {
    const GridLab p = sL[i];
    const int32_t base = __builtin_amdgcn_readfirstlane(p.base);
    const int32_t a = __builtin_amdgcn_readfirstlane(p.a);
    const int32_t b = __builtin_amdgcn_readfirstlane(p.b);
    const int32_t kind = __builtin_amdgcn_readfirstlane(p.kind);
    if (kind == 2) {
      const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane(p.c);
      const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane(p.r);
#pragma unroll
      for (int k = 0; k < kGPer; ++k)
        acc[k] = acc[k] + sD[base + (int32_t)(((uint32_t)(b + j[k]) / (uint32_t)a + c) % r)];
    } else if (kind == 1) {
#pragma unroll
      for (int k = 0; k < kGPer; ++k)
        acc[k] = acc[k] + sD[base + (int32_t)((uint32_t)(b + j[k]) / (uint32_t)a)];
    } else if (!Onto || kind == 0) {
#pragma unroll
      for (int k = 0; k < kGPer; ++k) acc[k] = acc[k] + sD[base + (j[k] >= a ? 1 : 0)];
    }
  }
#pragma unroll
  for (int k = 0; k < kGPer; ++k) {
    const int row = (int)threadIdx.x + k * kGBS;
    if (row < nv) S[t0 + row] = acc[k];
  }
}
}  // namespace
}  // namespace tpe

using namespace tpe;

namespace {
template <bool Onto>
int grid_fold(const char* fn, const double* bl, const double* al, const int64_t* host_off,
              const int64_t* host_radix, int n_labels, int64_t row_begin, int64_t n_rows,
              double* S_out, void* stream) {
  if (n_labels < 0 || n_labels > kGridMax) {
    set_error("%s: n_labels=%d outside [0, %d]", fn, n_labels, kGridMax);
    return TPE_E_ARG;
  }
  if (row_begin < 0 || n_rows < 0) {
    set_error("%s: row_begin=%lld n_rows=%lld", fn, (long long)row_begin, (long long)n_rows);
    return TPE_E_ARG;
  }
  if (n_labels > 0 && (!host_off || !host_radix)) {
    set_error("%s: null pointer (host_off / host_radix)", fn);
    return TPE_E_ARG;
  }
  GridArgs A;
  A.n = n_labels;
  int64_t rows = 1;  // of the block
  for (int i = 0; i < kGridMax; ++i) {
    A.off[i] = i < n_labels ? host_off[i] : 0;
    A.radix[i] = i < n_labels ? host_radix[i] : 1;
    if (A.radix[i] < 1) {
      set_error("%s: label %d has radix %lld < 1", fn, i, (long long)A.radix[i]);
      return TPE_E_ARG;
    }
    if (rows > INT64_MAX / A.radix[i]) {
      set_error("%s: the block's row count overflows int64 at label %d", fn, i);
      return TPE_E_ARG;
    }
    rows *= A.radix[i];
  }
  if (row_begin > rows || n_rows > rows - row_begin) {
    set_error("%s: rows [%lld, %lld + %lld) leave the block of %lld rows", fn,
              (long long)row_begin, (long long)row_begin, (long long)n_rows, (long long)rows);
    return TPE_E_ARG;
  }
  if (n_rows == 0) return TPE_OK;
  if (!S_out || (n_labels > 0 && (!bl || !al))) {
    set_error("%s: null pointer", fn);
    return TPE_E_ARG;
  }
  const int64_t tiles = (n_rows + kGTile - 1) / kGTile;
  if (tiles > 2147483647) {
    set_error("%s: n_rows=%lld does not fit a launch", fn, (long long)n_rows);
    return TPE_E_ARG;
  }
  hipLaunchKernelGGL(k_grid_fold<Onto>, dim3((unsigned)tiles), dim3(kGBS), 0,
                     (hipStream_t)stream, bl, al, A, row_begin, n_rows, S_out);
  return check_launch(fn);
}
}  // namespace

extern "C" int tpe_grid_fold(const double* bl, const double* al, const int64_t* host_off,
                             const int64_t* host_radix, int n_labels, int64_t row_begin,
                             int64_t n_rows, double* S_out, void* stream) {
  return grid_fold<false>("tpe_grid_fold", bl, al, host_off, host_radix, n_labels, row_begin,
                          n_rows, S_out, stream);
}

extern "C" int tpe_grid_fold_onto(const double* bl, const double* al, const int64_t* host_off,
                                  const int64_t* host_radix, int n_labels, int64_t row_begin,
                                  int64_t n_rows, double* S, void* stream) {
  return grid_fold<true>("tpe_grid_fold_onto", bl, al, host_off, host_radix, n_labels, row_begin,
                         n_rows, S, stream);
}
