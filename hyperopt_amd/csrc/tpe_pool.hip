// tpe_pool.hip -- ranking a fixed pool of configurations (tpe.suggest_from_pool).
//
// A pool is P configurations resident in HBM, one contiguous fp64 column per
// label plus one activity byte per (label, row).  The exact fp64 scorers read a
// column as their injected candidates and leave log l(c) and log g(c) per row;
// the two kernels here turn those into a ranking:
//
//   tpe_pool_fold   S[r] = sum over the labels active in row r, in label order,
//                   of (log l - log g): the joint criterion of broadcast_best
//                   (tpe.py:649-658) over whole configurations.  One thread per
//                   row adds its labels one after the other in fp64
//                   (-ffp-contract=off), so numpy replays the bits.
//   tpe_pool_topk   the k first untaken rows in np.argmax order: larger S
//                   first, NaN before everything, equal scores (-0.0 == +0.0)
//                   to the smaller row.
//
// Selection.  key(r) = ~order_key(S[r]) is a 64-bit integer whose ascending
// order is that order (NaN -> 1, the smallest).  A most-significant-digit
// radix select, 8 bits per pass, finds the key T of the k-th row: every tile
// of 4096 rows histograms its digit in LDS and adds its 256 counts to the
// global bins (integer adds: the sums do not depend on the order), one thread
// then picks the digit that holds the k-th row.  Rows with key < T are all
// selected; of the rows with key == T the first k_rem in row order are.  Per
// tile counts, one exclusive scan over the tiles and an in-tile scan in row
// order give every selected row its slot in a candidate list without atomics;
// the list is then ranked by counting, per candidate, the candidates that
// precede it in (key, row) order -- O(k^2) compares from LDS, exact, and the
// rank is the output position.  Nothing depends on block scheduling.
#include "tpe_common.hpp"

namespace tpe {
namespace {
constexpr int kPBS = 256;               // threads per block
constexpr int kPTile = 4096;            // rows per selection tile
constexpr int kPPer = kPTile / kPBS;    // rows per thread and tile
constexpr int kPBins = 256;             // 8 bits per pass
constexpr int kPPasses = 8;
constexpr int kFoldMax = 16;            // labels per fold launch

struct FoldArgs {
  int64_t off[kFoldMax];  // first log-density of the label in bl / al
  int64_t col[kFoldMax];  // the label's column (activity, terms)
  int n;
};

__global__ __launch_bounds__(kPBS) void k_pool_fold(const double* __restrict__ bl,
                                                    const double* __restrict__ al, FoldArgs A,
                                                    const uint8_t* __restrict__ active,
                                                    int64_t ld, int64_t n_rows, int init,
                                                    double* __restrict__ S,
                                                    double* __restrict__ terms,
                                                    int64_t terms_ld) {
  const int64_t r = (int64_t)blockIdx.x * kPBS + threadIdx.x;
  if (r >= n_rows) return;
  double s = init ? 0.0 : S[r];
  for (int i = 0; i < A.n; ++i) {
    const bool on = active[A.col[i] * ld + r] != 0;
    const double t = bl[A.off[i] + r] - al[A.off[i] + r];
    if (on) s = s + t;  // an inactive label is skipped, not added as zero
    if (terms) terms[A.col[i] * terms_ld + r] = on ? t : __longlong_as_double(0x7FF8000000000000ll);
  }
  S[r] = s;
}

// ascending pool_key = rank order (larger score first, NaN first)
__device__ __forceinline__ uint64_t pool_key(double v) { return ~order_key(v); }

struct PoolCtl {
  uint64_t prefix, mask;  // digits of the k-th key decided so far
  int64_t k_rem;          // rank still to find inside the current bin (1-based count)
  int64_t k_eff;          // rows selected: min(k, untaken rows)
  int64_t n_less;         // after the last pass: selected rows with key < T
  int64_t pad_[3];
};

__global__ void k_pool_init(PoolCtl* ctl, unsigned long long* hist, int64_t k) {
  hist[threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    ctl->prefix = ctl->mask = 0;
    ctl->k_rem = ctl->k_eff = k;
    ctl->n_less = 0;
  }
}

__global__ __launch_bounds__(kPBS) void k_pool_hist(const double* __restrict__ score,
                                                    const uint8_t* __restrict__ taken,
                                                    int64_t n_rows, int pass,
                                                    const PoolCtl* __restrict__ ctl,
                                                    unsigned long long* __restrict__ hist) {
  __shared__ uint32_t lh[kPBins];
  const uint64_t prefix = ctl->prefix, mask = ctl->mask;
  const int shift = 64 - 8 * (pass + 1);
  lh[threadIdx.x] = 0;
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * kPTile;
#pragma unroll 4
  for (int i = 0; i < kPPer; ++i) {
    const int64_t r = r0 + (int64_t)i * kPBS + threadIdx.x;
    if (r < n_rows && !taken[r]) {
      const uint64_t key = pool_key(score[r]);
      if ((key & mask) == prefix) atomicAdd(&lh[(key >> shift) & (kPBins - 1)], 1u);
    }
  }
  __syncthreads();
  const uint32_t c = lh[threadIdx.x];
  if (c) atomicAdd(&hist[threadIdx.x], (unsigned long long)c);
}

// one thread: the digit of the k-th key in this pass's bins; the bins are
// zeroed for the next pass
__global__ void k_pool_pick(int pass, PoolCtl* ctl, unsigned long long* hist) {
  if (threadIdx.x != 0) return;
  int64_t k_rem = ctl->k_rem;
  if (pass == 0) {
    int64_t total = 0;
    for (int d = 0; d < kPBins; ++d) total += (int64_t)hist[d];
    if (k_rem > total) k_rem = total;
    ctl->k_eff = k_rem;
  }
  if (k_rem > 0) {
    int64_t cum = 0;
    int digit = kPBins - 1;
    for (int d = 0; d < kPBins; ++d) {
      const int64_t h = (int64_t)hist[d];
      if (cum + h >= k_rem) {
        digit = d;
        break;
      }
      cum += h;
    }
    const int shift = 64 - 8 * (pass + 1);
    k_rem -= cum;
    ctl->prefix |= (uint64_t)digit << shift;
    ctl->mask |= (uint64_t)(kPBins - 1) << shift;
  }
  ctl->k_rem = k_rem;
  if (pass == kPPasses - 1) ctl->n_less = ctl->k_eff - k_rem;
  for (int d = 0; d < kPBins; ++d) hist[d] = 0;
}

// per tile: untaken rows with key < T and with key == T
__global__ __launch_bounds__(kPBS) void k_pool_count(const double* __restrict__ score,
                                                     const uint8_t* __restrict__ taken,
                                                     int64_t n_rows,
                                                     const PoolCtl* __restrict__ ctl,
                                                     int64_t* __restrict__ tile_cnt) {
  __shared__ int sl[kPBS], se[kPBS];
  const uint64_t T = ctl->prefix;
  const int64_t r0 = (int64_t)blockIdx.x * kPTile;
  int nl = 0, ne = 0;
  if (ctl->k_eff > 0) {
#pragma unroll 4
    for (int i = 0; i < kPPer; ++i) {
      const int64_t r = r0 + (int64_t)i * kPBS + threadIdx.x;
      if (r < n_rows && !taken[r]) {
        const uint64_t key = pool_key(score[r]);
        nl += key < T;
        ne += key == T;
      }
    }
  }
  sl[threadIdx.x] = nl;
  se[threadIdx.x] = ne;
  __syncthreads();
  for (int off = kPBS / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) {
      sl[threadIdx.x] += sl[threadIdx.x + off];
      se[threadIdx.x] += se[threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    tile_cnt[2 * (int64_t)blockIdx.x] = sl[0];
    tile_cnt[2 * (int64_t)blockIdx.x + 1] = se[0];
  }
}

// one block: the tile counts become exclusive offsets, in tile order
__global__ __launch_bounds__(kPBS) void k_pool_scan(int64_t* __restrict__ tile_cnt,
                                                    int64_t n_tiles) {
  __shared__ int64_t sl[kPBS], se[kPBS];
  const int64_t per = (n_tiles + kPBS - 1) / kPBS;
  const int64_t a = threadIdx.x * per;
  const int64_t b = a + per < n_tiles ? a + per : n_tiles;
  int64_t nl = 0, ne = 0;
  for (int64_t t = a; t < b; ++t) {
    nl += tile_cnt[2 * t];
    ne += tile_cnt[2 * t + 1];
  }
  sl[threadIdx.x] = nl;
  se[threadIdx.x] = ne;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t cl = 0, ce = 0;
    for (int i = 0; i < kPBS; ++i) {
      const int64_t l = sl[i], e = se[i];
      sl[i] = cl;
      se[i] = ce;
      cl += l;
      ce += e;
    }
  }
  __syncthreads();
  nl = sl[threadIdx.x];
  ne = se[threadIdx.x];
  for (int64_t t = a; t < b; ++t) {
    const int64_t l = tile_cnt[2 * t], e = tile_cnt[2 * t + 1];
    tile_cnt[2 * t] = nl;
    tile_cnt[2 * t + 1] = ne;
    nl += l;
    ne += e;
  }
}

// the selected rows into the candidate list: rows with key < T at
// [0, n_less) in row order, then the first k_rem rows with key == T.  Thread
// t of a tile owns its rows [t * kPPer, (t + 1) * kPPer): row order is thread
// order, so an exclusive scan over the threads' counts places every row.
__global__ __launch_bounds__(kPBS) void k_pool_gather(const double* __restrict__ score,
                                                      const uint8_t* __restrict__ taken,
                                                      int64_t n_rows,
                                                      const PoolCtl* __restrict__ ctl,
                                                      const int64_t* __restrict__ tile_off,
                                                      int64_t cap,
                                                      uint64_t* __restrict__ cand_key,
                                                      int64_t* __restrict__ cand_row) {
  __shared__ int sl[kPBS], se[kPBS];
  const uint64_t T = ctl->prefix;
  const int64_t k_eff = ctl->k_eff, k_rem = ctl->k_rem, n_less = ctl->n_less;
  if (k_eff <= 0) return;
  const int64_t r0 = (int64_t)blockIdx.x * kPTile + (int64_t)threadIdx.x * kPPer;
  uint64_t key[kPPer];
  uint32_t less = 0, eq = 0;  // bit i: row r0 + i
#pragma unroll
  for (int i = 0; i < kPPer; ++i) {
    const int64_t r = r0 + i;
    key[i] = 0;
    if (r < n_rows && !taken[r]) {
      key[i] = pool_key(score[r]);
      less |= (uint32_t)(key[i] < T) << i;
      eq |= (uint32_t)(key[i] == T) << i;
    }
  }
  sl[threadIdx.x] = __popc(less);
  se[threadIdx.x] = __popc(eq);
  __syncthreads();
  if (threadIdx.x == 0) {
    int cl = 0, ce = 0;
    for (int i = 0; i < kPBS; ++i) {
      const int l = sl[i], e = se[i];
      sl[i] = cl;
      se[i] = ce;
      cl += l;
      ce += e;
    }
  }
  __syncthreads();
  int64_t pl = tile_off[2 * (int64_t)blockIdx.x] + sl[threadIdx.x];
  int64_t pe = tile_off[2 * (int64_t)blockIdx.x + 1] + se[threadIdx.x];
#pragma unroll
  for (int i = 0; i < kPPer; ++i) {
    int64_t pos = -1;
    if ((less >> i) & 1u) {
      pos = pl++;
    } else if ((eq >> i) & 1u) {
      if (pe < k_rem) pos = n_less + pe;
      ++pe;
    }
    if (pos >= 0 && pos < k_eff && pos < cap) {
      cand_key[pos] = key[i];
      cand_row[pos] = r0 + i;
    }
  }
}

// rank by counting: out[rank] = row, rank = candidates before it in (key, row)
__global__ __launch_bounds__(kPBS) void k_pool_rank(const PoolCtl* __restrict__ ctl,
                                                    const uint64_t* __restrict__ cand_key,
                                                    const int64_t* __restrict__ cand_row,
                                                    int64_t cap, int64_t* __restrict__ out_rows,
                                                    int64_t* __restrict__ out_count) {
  __shared__ uint64_t sk[kPBS];
  __shared__ int64_t sr[kPBS];
  int64_t n = ctl->k_eff;
  if (n > cap) n = cap;
  if (blockIdx.x == 0 && threadIdx.x == 0 && out_count) *out_count = n;
  const int64_t i = (int64_t)blockIdx.x * kPBS + threadIdx.x;
  if ((int64_t)blockIdx.x * kPBS >= n) return;  // (the whole block)
  const bool mine = i < n;
  const uint64_t ki = mine ? cand_key[i] : 0;
  const int64_t ri = mine ? cand_row[i] : 0;
  int64_t rank = 0;
  for (int64_t j0 = 0; j0 < n; j0 += kPBS) {
    const int64_t j = j0 + threadIdx.x;
    __syncthreads();
    sk[threadIdx.x] = j < n ? cand_key[j] : ~0ull;
    sr[threadIdx.x] = j < n ? cand_row[j] : INT64_MAX;
    __syncthreads();
    const int m = (int)(n - j0 < kPBS ? n - j0 : kPBS);
    for (int q = 0; q < m; ++q) rank += (sk[q] < ki) || (sk[q] == ki && sr[q] < ri);
  }
  if (mine && rank < n) out_rows[rank] = ri;
}

inline int64_t pool_tiles(int64_t n_rows) { return (n_rows + kPTile - 1) / kPTile; }
constexpr int64_t kCtlBytes = 64, kHistBytes = 8 * kPBins;
static_assert(sizeof(PoolCtl) == kCtlBytes, "PoolCtl is the scratch's first 64 bytes");

// byte offsets of a call's scratch: tpe_pool_topk, its size query and
// tpe_pool_topk_layout all read them here
struct PoolLayout {
  int64_t n_tiles, kk;  // tiles of kPTile rows; candidate slots, min(k, n_rows)
  int64_t ctl, hist, tile, cand_key, cand_row, total;
};

inline PoolLayout pool_layout(int64_t n_rows, int64_t k) {
  PoolLayout p;
  p.n_tiles = pool_tiles(n_rows);
  p.kk = k < n_rows ? k : n_rows;
  p.ctl = 0;
  p.hist = p.ctl + kCtlBytes;
  p.tile = p.hist + kHistBytes;
  p.cand_key = p.tile + 16 * p.n_tiles;
  p.cand_row = p.cand_key + 8 * p.kk;
  p.total = p.cand_row + 8 * p.kk;
  return p;
}
}  // namespace
}  // namespace tpe

using namespace tpe;

extern "C" int tpe_pool_fold(const double* bl, const double* al, const int64_t* host_off,
                             const int64_t* host_col, int n_labels, const uint8_t* active,
                             int64_t ld, int64_t n_rows, int init, double* S, double* terms,
                             int64_t terms_ld, void* stream) {
  if (n_rows < 0 || n_labels < 0 || ld < 0) {
    set_error("tpe_pool_fold: n_rows=%lld n_labels=%d ld=%lld", (long long)n_rows, n_labels,
              (long long)ld);
    return TPE_E_ARG;
  }
  if (n_rows == 0 || (n_labels == 0 && !init)) return TPE_OK;
  if (!S || (n_labels > 0 && (!bl || !al || !host_off || !host_col || !active))) {
    set_error("tpe_pool_fold: null pointer");
    return TPE_E_ARG;
  }
  if (n_rows > (int64_t)2147483647 * kPBS || (n_labels > 0 && ld < n_rows) ||
      (terms && terms_ld < n_rows)) {
    set_error("tpe_pool_fold: n_rows=%lld does not fit ld=%lld / terms_ld=%lld / a launch",
              (long long)n_rows, (long long)ld, (long long)terms_ld);
    return TPE_E_ARG;
  }
  for (int i = 0; i < n_labels; ++i) {
    if (host_off[i] < 0 || host_col[i] < 0) {
      set_error("tpe_pool_fold: label %d has a negative offset or column", i);
      return TPE_E_ARG;
    }
  }
  const dim3 grid((unsigned)((n_rows + kPBS - 1) / kPBS));
  int done = 0;
  do {  // (once with no label and init: S = 0)
    FoldArgs A;
    A.n = n_labels - done < kFoldMax ? n_labels - done : kFoldMax;
    for (int i = 0; i < kFoldMax; ++i) {
      A.off[i] = i < A.n ? host_off[done + i] : 0;
      A.col[i] = i < A.n ? host_col[done + i] : 0;
    }
    hipLaunchKernelGGL(k_pool_fold, grid, dim3(kPBS), 0, (hipStream_t)stream, bl, al, A, active,
                       ld, n_rows, (init && done == 0) ? 1 : 0, S, terms, terms_ld);
    const int rc = check_launch("tpe_pool_fold");
    if (rc != TPE_OK) return rc;
    done += A.n;
  } while (done < n_labels);
  return TPE_OK;
}

extern "C" int64_t tpe_pool_topk_scratch_bytes(int64_t n_rows, int64_t k) {
  if (n_rows < 0 || k < 0) return -1;
  return pool_layout(n_rows, k).total;
}

extern "C" int tpe_pool_topk_layout(int64_t n_rows, int64_t k, int64_t* out, int n) {
  if (n_rows < 0 || k < 0 || n < 0 || (n > 0 && !out)) {
    set_error("tpe_pool_topk_layout: n_rows=%lld k=%lld n=%d", (long long)n_rows, (long long)k,
              n);
    return -1;
  }
  const PoolLayout p = pool_layout(n_rows, k);
  const int64_t v[7] = {p.ctl, p.hist, p.tile, p.cand_key, p.cand_row, p.total, kPTile};
  const int m = n < 7 ? n : 7;
  for (int i = 0; i < m; ++i) out[i] = v[i];
  return m;
}

extern "C" int tpe_pool_topk(const double* score, const uint8_t* taken, int64_t n_rows, int64_t k,
                             int64_t* out_rows, int64_t* out_count, void* scratch,
                             void* stream) {
  if (n_rows < 0 || k < 0) {
    set_error("tpe_pool_topk: n_rows=%lld k=%lld", (long long)n_rows, (long long)k);
    return TPE_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  if (n_rows == 0 || k == 0) {
    if (out_count && hipMemsetAsync(out_count, 0, sizeof(int64_t), st) != hipSuccess) {
      set_error("tpe_pool_topk: hipMemsetAsync failed");
      return TPE_E_LAUNCH;
    }
    return TPE_OK;
  }
  if (!score || !taken || !out_rows || !out_count || !scratch) {
    set_error("tpe_pool_topk: null pointer");
    return TPE_E_ARG;
  }
  const PoolLayout lay = pool_layout(n_rows, k);
  const int64_t n_tiles = lay.n_tiles, kk = lay.kk;
  if (n_tiles > 2147483647) {
    set_error("tpe_pool_topk: n_rows=%lld does not fit a launch", (long long)n_rows);
    return TPE_E_ARG;
  }
  uint8_t* ws = static_cast<uint8_t*>(scratch);
  PoolCtl* ctl = reinterpret_cast<PoolCtl*>(ws + lay.ctl);
  unsigned long long* hist = reinterpret_cast<unsigned long long*>(ws + lay.hist);
  int64_t* tile_cnt = reinterpret_cast<int64_t*>(ws + lay.tile);
  uint64_t* cand_key = reinterpret_cast<uint64_t*>(ws + lay.cand_key);
  int64_t* cand_row = reinterpret_cast<int64_t*>(ws + lay.cand_row);
  const dim3 tiles((unsigned)n_tiles), bs(kPBS);
  hipLaunchKernelGGL(k_pool_init, dim3(1), dim3(kPBins), 0, st, ctl, hist, kk);
  for (int pass = 0; pass < kPPasses; ++pass) {
    hipLaunchKernelGGL(k_pool_hist, tiles, bs, 0, st, score, taken, n_rows, pass, ctl, hist);
    hipLaunchKernelGGL(k_pool_pick, dim3(1), dim3(64), 0, st, pass, ctl, hist);
  }
  hipLaunchKernelGGL(k_pool_count, tiles, bs, 0, st, score, taken, n_rows, ctl, tile_cnt);
  hipLaunchKernelGGL(k_pool_scan, dim3(1), bs, 0, st, tile_cnt, n_tiles);
  hipLaunchKernelGGL(k_pool_gather, tiles, bs, 0, st, score, taken, n_rows, ctl, tile_cnt, kk,
                     cand_key, cand_row);
  hipLaunchKernelGGL(k_pool_rank, dim3((unsigned)((kk + kPBS - 1) / kPBS)), bs, 0, st, ctl,
                     cand_key, cand_row, kk, out_rows, out_count);
  return check_launch("tpe_pool_topk");
}
