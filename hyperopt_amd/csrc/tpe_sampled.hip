// tpe_sampled.hip -- a pool sampled from the posterior (tpe.Pool.sample).
//
// The exact fp64 scorers draw candidate r of every label's stream and leave its
// value and its log l / log g on the device.  Reading candidate r of every
// label as configuration r makes the draws a pool (tpe_pool.hip); the three
// kernels here are what that step needs besides the fold and the top-k:
//
//   tpe_rows_active  which labels are live in each row, from the row's own
//                    selector values: the space's liveness as a program of
//                    clauses (Domain.live_program), one thread per row.
//   tpe_pool_ranges  per label the (min, max) of its live finite values, the
//                    range a later re-score of the columns names (cand_dev).
//   tpe_pool_take    the winners' rows as (k, n_labels) blocks: the only
//                    per-row data that goes back to the host.
//
// Nothing here adds floating-point numbers; the counts and the extrema are
// integer atomics (sums, min / max of order-preserving keys), so no result
// depends on block scheduling.
#include "tpe_common.hpp"

namespace tpe {
namespace {
constexpr int kSBS = 256;                 // threads per block
constexpr int kSWaves = kSBS / kWave;
constexpr int kRangePer = 8;              // rows per thread of k_pool_ranges
constexpr int kRangeLabels = 64;          // labels per k_pool_ranges launch (one mask word)

// the liveness program, in the kernel's arguments (limits: tpe_hip.h)
struct CondProgram {
  uint16_t label_off[TPE_COND_MAX_LABELS + 1];
  uint16_t clause_off[TPE_COND_MAX_CLAUSES + 1];
  tpe_cond_term terms[TPE_COND_MAX_TERMS];
};

__global__ __launch_bounds__(kSBS) void k_rows_active(const double* __restrict__ vals, int64_t ld,
                                                      int64_t n_rows, int n_labels, int n_clauses,
                                                      int n_terms, CondProgram P,
                                                      uint8_t* __restrict__ active,
                                                      unsigned long long* __restrict__ n_active) {
  __shared__ uint16_t s_label[TPE_COND_MAX_LABELS + 1];
  __shared__ uint16_t s_clause[TPE_COND_MAX_CLAUSES + 1];
  __shared__ tpe_cond_term s_term[TPE_COND_MAX_TERMS];
  __shared__ uint32_t s_cnt[TPE_COND_MAX_LABELS];
  for (int i = threadIdx.x; i <= n_labels; i += kSBS) s_label[i] = P.label_off[i];
  for (int i = threadIdx.x; i <= n_clauses; i += kSBS) s_clause[i] = P.clause_off[i];
  for (int i = threadIdx.x; i < n_terms; i += kSBS) s_term[i] = P.terms[i];
  for (int i = threadIdx.x; i < n_labels; i += kSBS) s_cnt[i] = 0;
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * kSBS + threadIdx.x;
  const bool in = r < n_rows;
  for (int j = 0; j < n_labels; ++j) {
    bool live = false;
    if (in) {
      for (int c = s_label[j]; c < s_label[j + 1] && !live; ++c) {
        bool ok = true;
        for (int t = s_clause[c]; t < s_clause[c + 1] && ok; ++t) {
          const tpe_cond_term T = s_term[t];
          // (rint: llrint's rounding, and false for NaN / inf)
          ok = rint(vals[(int64_t)T.col * ld + r]) == (double)T.value;
        }
        live = ok;
      }
      active[(int64_t)j * ld + r] = live ? 1 : 0;
    }
    const unsigned long long m = __ballot(live);
    if (lane_id() == 0 && m) atomicAdd(&s_cnt[j], (uint32_t)__popcll(m));
  }
  __syncthreads();
  for (int j = threadIdx.x; j < n_labels; j += kSBS) {
    const uint32_t c = s_cnt[j];
    if (c) atomicAdd(&n_active[j], (unsigned long long)c);
  }
}

// ascending integer order of the doubles, -0.0 below +0.0 (the extrema of a
// set are then the same in every order of arrival)
__device__ __forceinline__ uint64_t total_key(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
constexpr uint64_t kKeyNone = ~0ull;  // min of nothing (no finite value has this key)

__global__ void k_ranges_init(unsigned long long* __restrict__ out, int n_labels) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n_labels) {
    out[2 * j] = kKeyNone;
    out[2 * j + 1] = 0;
  }
}

// grid (row tiles, labels of this launch): the block's live finite values of
// label j0 + blockIdx.y (bit of `positive`: only those > 0) into the label's
// (min key, max key)
__global__ __launch_bounds__(kSBS) void k_pool_ranges(const double* __restrict__ vals,
                                                      const uint8_t* __restrict__ active,
                                                      int64_t ld, int64_t n_rows, int j0,
                                                      uint64_t positive,
                                                      unsigned long long* __restrict__ out) {
  __shared__ uint64_t s_lo[kSWaves], s_hi[kSWaves];
  const int j = j0 + blockIdx.y;
  const bool pos = (positive >> blockIdx.y) & 1ull;
  const double* col = vals + (int64_t)j * ld;
  const uint8_t* act = active + (int64_t)j * ld;
  uint64_t lo = kKeyNone, hi = 0;
  const int64_t r0 = (int64_t)blockIdx.x * (kSBS * kRangePer) + threadIdx.x;
#pragma unroll
  for (int i = 0; i < kRangePer; ++i) {
    const int64_t r = r0 + (int64_t)i * kSBS;
    if (r < n_rows && act[r]) {
      const double v = col[r];
      if (fabs(v) < INFINITY && (!pos || v > 0.0)) {  // (false for NaN)
        const uint64_t k = total_key(v);
        lo = k < lo ? k : lo;
        hi = k > hi ? k : hi;
      }
    }
  }
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1) {
    const uint64_t ol = (uint64_t)__shfl_xor((unsigned long long)lo, off, kWave);
    const uint64_t oh = (uint64_t)__shfl_xor((unsigned long long)hi, off, kWave);
    lo = ol < lo ? ol : lo;
    hi = oh > hi ? oh : hi;
  }
  if (lane_id() == 0) {
    s_lo[threadIdx.x / kWave] = lo;
    s_hi[threadIdx.x / kWave] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kSWaves; ++w) {
      lo = s_lo[w] < lo ? s_lo[w] : lo;
      hi = s_hi[w] > hi ? s_hi[w] : hi;
    }
    if (lo != kKeyNone) {  // (then hi is a value's key too)
      atomicMin(&out[2 * j], (unsigned long long)lo);
      atomicMax(&out[2 * j + 1], (unsigned long long)hi);
    }
  }
}

// keys back to doubles, in place; a label without a value: (+inf, -inf)
__global__ void k_ranges_finish(unsigned long long* __restrict__ out, int n_labels) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_labels) return;
  const uint64_t lo = out[2 * j], hi = out[2 * j + 1];
  double* o = reinterpret_cast<double*>(out);
  if (lo == kKeyNone) {
    o[2 * j] = INFINITY;
    o[2 * j + 1] = -INFINITY;
  } else {
    o[2 * j] = __longlong_as_double((long long)((lo >> 63) ? (lo & ~(1ull << 63)) : ~lo));
    o[2 * j + 1] = __longlong_as_double((long long)((hi >> 63) ? (hi & ~(1ull << 63)) : ~hi));
  }
}

// one thread per (picked row, label); a row outside [0, ld) reads nothing
__global__ __launch_bounds__(kSBS) void k_pool_take(const double* __restrict__ vals,
                                                    const uint8_t* __restrict__ active,
                                                    int64_t ld, int n_labels,
                                                    const int64_t* __restrict__ rows, int64_t k,
                                                    double* __restrict__ out_vals,
                                                    uint8_t* __restrict__ out_active) {
  const int64_t e = (int64_t)blockIdx.x * kSBS + threadIdx.x;
  if (e >= k * n_labels) return;
  const int64_t i = e / n_labels;
  const int j = (int)(e - i * n_labels);
  const int64_t r = rows[i];
  const bool ok = r >= 0 && r < ld;
  out_vals[e] = ok ? vals[(int64_t)j * ld + r] : __longlong_as_double(0x7FF8000000000000ll);
  out_active[e] = ok ? active[(int64_t)j * ld + r] : 0;
}
}  // namespace
}  // namespace tpe

using namespace tpe;

extern "C" int tpe_sampled_struct_sizes(int32_t* out, int n) {
  const int32_t s[1] = {(int32_t)sizeof(tpe_cond_term)};
  for (int i = 0; i < n && i < 1; ++i) out[i] = s[i];
  return 1;
}

extern "C" int tpe_rows_active(const double* vals, int64_t ld, int64_t n_rows, int n_labels,
                               const int32_t* host_label_off, const int32_t* host_clause_off,
                               const tpe_cond_term* host_terms, int n_terms, uint8_t* active,
                               int64_t* n_active, void* stream) {
  if (n_rows < 0 || n_labels < 0 || n_terms < 0 || ld < 0) {
    set_error("tpe_rows_active: n_rows=%lld n_labels=%d n_terms=%d ld=%lld", (long long)n_rows,
              n_labels, n_terms, (long long)ld);
    return TPE_E_ARG;
  }
  if (n_labels == 0) return TPE_OK;
  if (!host_label_off || !host_clause_off || (n_terms > 0 && !host_terms)) {
    set_error("tpe_rows_active: null pointer (program)");
    return TPE_E_ARG;
  }
  if (n_labels > TPE_COND_MAX_LABELS || n_terms > TPE_COND_MAX_TERMS) {
    set_error("tpe_rows_active: program of %d labels / %d terms over the limit (%d / %d)",
              n_labels, n_terms, TPE_COND_MAX_LABELS, TPE_COND_MAX_TERMS);
    return TPE_E_UNSUPPORTED;
  }
  if (host_label_off[0] != 0) {
    set_error("tpe_rows_active: label_off[0]=%d", host_label_off[0]);
    return TPE_E_ARG;
  }
  for (int j = 0; j < n_labels; ++j) {
    if (host_label_off[j + 1] < host_label_off[j]) {
      set_error("tpe_rows_active: label_off decreases at label %d", j);
      return TPE_E_ARG;
    }
  }
  const int n_clauses = host_label_off[n_labels];
  if (n_clauses > TPE_COND_MAX_CLAUSES) {
    set_error("tpe_rows_active: program of %d clauses over the limit (%d)", n_clauses,
              TPE_COND_MAX_CLAUSES);
    return TPE_E_UNSUPPORTED;
  }
  if (host_clause_off[0] != 0 || host_clause_off[n_clauses] != n_terms) {
    set_error("tpe_rows_active: clause_off spans [%d, %d], expected [0, %d]", host_clause_off[0],
              host_clause_off[n_clauses], n_terms);
    return TPE_E_ARG;
  }
  for (int c = 0; c < n_clauses; ++c) {
    if (host_clause_off[c + 1] < host_clause_off[c]) {
      set_error("tpe_rows_active: clause_off decreases at clause %d", c);
      return TPE_E_ARG;
    }
  }
  for (int t = 0; t < n_terms; ++t) {
    if (host_terms[t].col < 0 || host_terms[t].col >= n_labels) {
      set_error("tpe_rows_active: term %d names column %d outside [0, %d)", t, host_terms[t].col,
                n_labels);
      return TPE_E_ARG;
    }
  }
  if (n_rows == 0) return TPE_OK;
  if (!vals || !active || !n_active) {
    set_error("tpe_rows_active: null pointer");
    return TPE_E_ARG;
  }
  if (ld < n_rows || n_rows > (int64_t)2147483647 * kSBS) {
    set_error("tpe_rows_active: n_rows=%lld does not fit ld=%lld / a launch", (long long)n_rows,
              (long long)ld);
    return TPE_E_ARG;
  }
  CondProgram P;
  for (int j = 0; j <= TPE_COND_MAX_LABELS; ++j)
    P.label_off[j] = (uint16_t)(j <= n_labels ? host_label_off[j] : 0);
  for (int c = 0; c <= TPE_COND_MAX_CLAUSES; ++c)
    P.clause_off[c] = (uint16_t)(c <= n_clauses ? host_clause_off[c] : 0);
  for (int t = 0; t < TPE_COND_MAX_TERMS; ++t)
    P.terms[t] = t < n_terms ? host_terms[t] : tpe_cond_term{0, 0};
  hipLaunchKernelGGL(k_rows_active, dim3((unsigned)((n_rows + kSBS - 1) / kSBS)), dim3(kSBS), 0,
                     (hipStream_t)stream, vals, ld, n_rows, n_labels, n_clauses, n_terms, P,
                     active, reinterpret_cast<unsigned long long*>(n_active));
  return check_launch("tpe_rows_active");
}

extern "C" int tpe_pool_ranges(const double* vals, const uint8_t* active, int64_t ld,
                               int64_t n_rows, int n_labels, const uint8_t* host_positive,
                               double* out, void* stream) {
  if (n_rows < 0 || n_labels < 0 || ld < 0) {
    set_error("tpe_pool_ranges: n_rows=%lld n_labels=%d ld=%lld", (long long)n_rows, n_labels,
              (long long)ld);
    return TPE_E_ARG;
  }
  if (n_labels == 0) return TPE_OK;
  if (!out || !host_positive || (n_rows > 0 && (!vals || !active))) {
    set_error("tpe_pool_ranges: null pointer");
    return TPE_E_ARG;
  }
  const int64_t tiles = (n_rows + kSBS * kRangePer - 1) / (kSBS * kRangePer);
  if (ld < n_rows || tiles > 2147483647) {
    set_error("tpe_pool_ranges: n_rows=%lld does not fit ld=%lld / a launch", (long long)n_rows,
              (long long)ld);
    return TPE_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(out);
  const dim3 per_label((unsigned)((n_labels + kSBS - 1) / kSBS));
  hipLaunchKernelGGL(k_ranges_init, per_label, dim3(kSBS), 0, st, keys, n_labels);
  for (int j0 = 0; j0 < n_labels && n_rows > 0; j0 += kRangeLabels) {
    const int nl = n_labels - j0 < kRangeLabels ? n_labels - j0 : kRangeLabels;
    uint64_t positive = 0;
    for (int i = 0; i < nl; ++i) positive |= (uint64_t)(host_positive[j0 + i] != 0) << i;
    hipLaunchKernelGGL(k_pool_ranges, dim3((unsigned)tiles, (unsigned)nl), dim3(kSBS), 0, st, vals,
                       active, ld, n_rows, j0, positive, keys);
  }
  hipLaunchKernelGGL(k_ranges_finish, per_label, dim3(kSBS), 0, st, keys, n_labels);
  return check_launch("tpe_pool_ranges");
}

extern "C" int tpe_pool_take(const double* vals, const uint8_t* active, int64_t ld, int n_labels,
                             const int64_t* rows, int64_t k, double* out_vals,
                             uint8_t* out_active, void* stream) {
  if (k < 0 || n_labels < 0 || ld < 0) {
    set_error("tpe_pool_take: k=%lld n_labels=%d ld=%lld", (long long)k, n_labels, (long long)ld);
    return TPE_E_ARG;
  }
  if (k == 0 || n_labels == 0) return TPE_OK;
  if (!vals || !active || !rows || !out_vals || !out_active) {
    set_error("tpe_pool_take: null pointer");
    return TPE_E_ARG;
  }
  const int64_t blocks = (k * n_labels + kSBS - 1) / kSBS;
  if (k > ((int64_t)1 << 40) || blocks > 2147483647) {
    set_error("tpe_pool_take: k=%lld rows of %d labels do not fit a launch", (long long)k,
              n_labels);
    return TPE_E_ARG;
  }
  hipLaunchKernelGGL(k_pool_take, dim3((unsigned)blocks), dim3(kSBS), 0, (hipStream_t)stream, vals,
                     active, ld, n_labels, rows, k, out_vals, out_active);
  return check_launch("tpe_pool_take");
}
