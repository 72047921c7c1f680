// tpe_fit.hip -- categorical pseudocount posteriors.
//
// Replaces the categorical posteriors of hyperopt/tpe.py:578-615 (randint /
// categorical / pchoice) with pyll/base.py:1053-1060 (bincount).  The Parzen
// fit of continuous labels is tpe_parzen.hip.
#include <algorithm>
#include <stdarg.h>
#include <stdio.h>

#include "tpe_common.hpp"
#include "tpe_fold.hpp"

namespace tpe {

namespace {
// ---------------------------------------------------------------------------
// categorical posteriors
// ---------------------------------------------------------------------------
// numpy's pairwise_sum for float64, so `pseudocounts / np.sum(pseudocounts)`
// is reproduced bit for bit.  np.sum reduces a contiguous array buffer by
// buffer: one pairwise sum up to kNpBuf elements, and past that the pairwise
// sums of the consecutive kNpBuf-element chunks added in order (np_sum).
constexpr int64_t kNpBuf = 8192;  // numpy's reduction buffer, in elements

__device__ double np_pw_leaf(const double* a, int64_t n) {
  if (n < 8) {
    double r = 0.0;
    for (int64_t i = 0; i < n; ++i) r += a[i];
    return r;
  }
  double r[8];
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  int64_t i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; ++j) r[j] += a[i + j];
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return res;
}

__device__ double np_pairwise_sum(const double* a, int64_t n) {
  if (n <= 128) return np_pw_leaf(a, n);
  struct Frame {
    int64_t s, n;
    double left;
    int st;
  };
  // (one thread sums; its explicit stack lives in LDS, not in scratch: a
  // private array here gave the calling kernel 1.5 KB of scratch per lane)
  __shared__ Frame stk[48];
  int sp = 0;
  stk[0] = Frame{0, n, 0.0, 0};
  double ret = 0.0;
  while (sp >= 0) {
    Frame& f = stk[sp];
    if (f.n <= 128) {
      ret = np_pw_leaf(a + f.s, f.n);
      --sp;
      continue;
    }
    int64_t n2 = f.n / 2;
    n2 -= n2 % 8;
    if (f.st == 0) {
      f.st = 1;
      stk[sp + 1] = Frame{f.s, n2, 0.0, 0};
      ++sp;
    } else if (f.st == 1) {
      f.left = ret;
      f.st = 2;
      stk[sp + 1] = Frame{f.s + n2, f.n - n2, 0.0, 0};
      ++sp;
    } else {
      ret = f.left + ret;
      --sp;
    }
  }
  return ret;
}

// np.sum of n contiguous doubles (called by one thread of the block)
__device__ double np_sum(const double* a, int64_t n) {
  double total = np_pairwise_sum(a, std::min(n, kNpBuf));
  for (int64_t s = kNpBuf; s < n; s += kNpBuf)
    total += np_pairwise_sum(a + s, std::min(n - s, kNpBuf));
  return total;
}

constexpr int kCatBS = 256;
constexpr int kCatWaves = kCatBS / kWave;

// Weighted counts, one wave per (segment, category): np.bincount's sum
// (pyll/base.py:1053-1060) adds the LF weights of a category's observations
// sequentially in observation order, fl(..fl(fl(c + w0) + w1)..), and the
// result must be that chain's bits.  The wave scans 64 observations per
// step, ballots the matches, and every matching lane writes its weight
// (computed in parallel) into the wave's LDS list at its rank; a full list
// is folded into the running count by fold_list (tpe_fold.hpp) -- the same
// bits as the serial chain, in a few wave-wide passes instead of one fp64 add
// latency per match (a 60 000-match category: ~0.45 ms serially).
constexpr int kCatList = 1024;  // weights buffered per wave before a fold

// a category's count into its pseudocount (lane 0 / thread 0 of its owner)
__device__ __forceinline__ void cat_pseudocount(const tpe_cat_seg& S, double* __restrict__ p,
                                                int k, double cnt) {
  double pseudo;
  if (S.mode == 0) {
    pseudo = cnt + S.prior_weight;  // tpe.py:589
  } else {
    const double pk = p[S.prior_p_off + k];
    pseudo = cnt + (double)S.n_cat * (S.prior_weight * pk);  // tpe.py:603
  }
  p[S.p_off + k] = pseudo;
}

__global__ __launch_bounds__(kCatBS) void k_cat_counts(const int64_t* __restrict__ obs,
                                                       const tpe_cat_seg* __restrict__ segs,
                                                       double* __restrict__ p) {
  __shared__ double s_list[kCatWaves][kCatList];
  const tpe_cat_seg& S = segs[blockIdx.y];
  const int k = blockIdx.x * kCatWaves + threadIdx.x / kWave;
  if (k >= S.n_cat) return;  // wave-uniform
  double* list = s_list[threadIdx.x / kWave];
  const int n = S.n_obs, lane = lane_id();
  const LfRamp lfw(n, S.lf);
  const uint64_t lt = (1ull << lane) - 1ull;
  double cnt = 0.0;
  int filled = 0;
  int64_t folded = 0;
  auto fold = [&]() {
    __builtin_amdgcn_wave_barrier();
    cnt = fold_list<8>(cnt, list, filled, folded, lane);
    filled = 0;
    __builtin_amdgcn_wave_barrier();
  };
  // kDepth tiles of 64 observations per step, the next step's loads issued
  // before this step's matches are listed (a latency-bound scan); the list
  // holds a whole step, so it is folded only between steps
  constexpr int kDepth = 16;
  static_assert(kDepth * kWave <= kCatList, "a step's matches fit the list");
  const int64_t* O = obs + S.obs_off;
  int64_t nxt[kDepth];
#pragma unroll
  for (int b = 0; b < kDepth; ++b) {
    const int i = b * kWave + lane;
    nxt[b] = i < n ? O[i] : -1;
  }
  for (int t0 = 0; t0 < n; t0 += kDepth * kWave) {
    int64_t cur[kDepth];
#pragma unroll
    for (int b = 0; b < kDepth; ++b) {
      cur[b] = nxt[b];
      const int i = t0 + (kDepth + b) * kWave + lane;
      nxt[b] = i < n ? O[i] : -1;
    }
    if (filled + kDepth * kWave > kCatList) fold();
#pragma unroll
    for (int b = 0; b < kDepth; ++b) {
      const bool hit = cur[b] == (int64_t)k;
      const uint64_t m = __ballot(hit);
      if (m == 0) continue;  // wave-uniform
      if (hit) list[filled + __popcll(m & lt)] = lfw.at(t0 + b * kWave + lane);
      filled += __popcll(m);
    }
  }
  fold();
  if (lane == 0) cat_pseudocount(S, p, k, cnt);
}

// The same counts read straight from the HBM history (the gathered lists'
// work folded in): one 1024-thread block per (segment, category) walks the
// rows in windows of kCHW (row order = tid order, as tpe_gather_obs lists
// them), a row being an observation of the segment when the label is active
// there and the row is on the segment's side of the split.  Waves 1-15 scan:
// one scan of the packed (observations << 16 | matches) counts per (tile,
// wave) gives every observation its position in the segment -- its LF
// weight -- and every match its rank in the window, the window's match
// weights going to LDS in order; wave 0 folds (fold_list) the previous
// window's weights meanwhile, from the other of two LDS buffers (the fold of
// a long chain is a serial-latency walk; the scan is load latency: they
// overlap).  A segment whose observation count differs from S.n_obs sets
// bit 4 of *err (tpe_gather_obs' rule).

// row i of a history walk: a member of the segment (active label, the
// segment's side of the split) and its category (-1: none of 0..n_cat-1)
__device__ __forceinline__ void cath_row(const double* __restrict__ V,
                                         const uint8_t* __restrict__ Ac,
                                         const int32_t* __restrict__ rows,
                                         const uint8_t* __restrict__ is_below, int64_t i,
                                         int64_t n_rows, uint8_t side, int64_t offset, int n_cat,
                                         bool& mem, int& cat) {
  mem = false;
  cat = -1;
  if (i < n_rows) {
    const int64_t r = rows ? (int64_t)rows[i] : i;
    const bool a = Ac[r] != 0;
    const double v = V[r];  // (read unconditionally: one latency, not two)
    mem = a && is_below[i] == side;
    const int64_t cv = (int64_t)v - offset;
    if (mem && cv >= 0 && cv < (int64_t)n_cat) cat = (int)cv;
  }
}

constexpr int kCHB = 1024;             // block
constexpr int kCHScan = kCHB / kWave - 1;  // scanning waves (wave 0 folds)
constexpr int kCHT = 8;                // rows per scanning thread per window
constexpr int kCHW = kCHScan * kWave * kCHT;  // rows per window (7 680)
constexpr int kCHSlots = kCHT * kCHScan;      // (tile, wave) counts per window
constexpr int kCHSE = 8;               // fold entries per lane (512 per pass; wider
                                       // passes measured slower: 16 +25 %, 32 +65 %)
static_assert(kCHSlots <= 2 * kWave, "the slot scan: two slots per lane of one wave");
static_assert(kCHW < (1 << 16), "packed 16-bit counts");

__global__ __launch_bounds__(kCHB) void k_cat_counts_hist(
    const double* __restrict__ vals, const uint8_t* __restrict__ active, int64_t ld,
    const int32_t* __restrict__ rows, int64_t n_rows, const uint8_t* __restrict__ is_below,
    const tpe_gather* __restrict__ gathers, const tpe_cat_seg* __restrict__ segs,
    double* __restrict__ p, int32_t* __restrict__ err) {
  __shared__ double s_w[2][kCHW];
  __shared__ uint32_t s_slot[2 * kWave];
  __shared__ uint32_t s_tot[2];  // per buffer: the window's packed totals
  const tpe_cat_seg S = segs[blockIdx.y];
  const int k = blockIdx.x;
  if (k >= S.n_cat) return;  // (block-uniform)
  const tpe_gather G = gathers[blockIdx.y];
  const double* __restrict__ V = vals + (int64_t)G.col * ld;
  const uint8_t* __restrict__ Ac = active + (int64_t)G.col * ld;
  const uint8_t side = G.below ? 1 : 0;
  const int lane = lane_id(), wid = threadIdx.x / kWave;
  const int sw = wid - 1;                   // scanning wave index (waves 1..)
  const int st = threadIdx.x - kWave;       // scanning thread index
  const uint64_t lt = (1ull << lane) - 1ull;
  const int n = S.n_obs;
  const LfRamp lfw(n, S.lf);
  double cnt = 0.0;     // (wave 0)
  int64_t folded = 0;  // (wave 0) matches folded so far
  int64_t carry = 0;   // (scanners) observations before the window
  const int64_t n_win = (n_rows + kCHW - 1) / kCHW;
  for (int64_t it = 0; it <= n_win; ++it) {  // (block-uniform; the last round only folds)
    const int buf = (int)(it & 1);
    const bool scan = it < n_win;
    bool mem[kCHT], hit[kCHT];
    uint32_t pre[kCHT];
    // ---- phase 0: scanners load and ballot window `it`; wave 0 folds window it - 1
    if (wid > 0 && scan) {
      const int64_t p0 = it * kCHW;
#pragma unroll
      for (int t = 0; t < kCHT; ++t) {
        int cat;
        cath_row(V, Ac, rows, is_below, p0 + (int64_t)t * (kCHScan * kWave) + st, n_rows, side,
                 G.offset, S.n_cat, mem[t], cat);
        hit[t] = cat == k;  // (0 <= k < n_cat)
      }
#pragma unroll
      for (int t = 0; t < kCHT; ++t) {
        const uint64_t bm = __ballot(mem[t]), bh = __ballot(hit[t]);
        pre[t] = ((uint32_t)__popcll(bm & lt) << 16) | (uint32_t)__popcll(bh & lt);
        if (lane == 0) s_slot[t * kCHScan + sw] = ((uint32_t)__popcll(bm) << 16) |
                                                  (uint32_t)__popcll(bh);
      }
    }
    if (wid == 0 && it > 0) {
      const int nh = (int)(s_tot[buf ^ 1] & 0xffffu);
      cnt = fold_list<kCHSE>(cnt, s_w[buf ^ 1], nh, folded, lane);
    }
    __syncthreads();
    if (!scan) break;
    // ---- phase 1: exclusive scan of the slots (tile-major, then wave: row
    // order) on wave 1, two slots per lane
    if (wid == 1) {
      const uint32_t c0 = 2 * lane < kCHSlots ? s_slot[2 * lane] : 0u;
      const uint32_t c1 = 2 * lane + 1 < kCHSlots ? s_slot[2 * lane + 1] : 0u;
      uint32_t incl = c0 + c1;
#pragma unroll
      for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)incl, o, kWave);
        if (lane >= o) incl += y;
      }
      const uint32_t ex = incl - (c0 + c1);
      if (2 * lane < kCHSlots) s_slot[2 * lane] = ex;
      if (2 * lane + 1 < kCHSlots) s_slot[2 * lane + 1] = ex + c0;
      if (lane == kWave - 1) s_tot[buf] = incl;
    }
    __syncthreads();
    // ---- phase 2: the window's match weights into s_w[buf], in order
    if (wid > 0) {
#pragma unroll
      for (int t = 0; t < kCHT; ++t) {
        if (hit[t]) {
          const uint32_t ex = s_slot[t * kCHScan + sw] + pre[t];
          s_w[buf][ex & 0xffffu] = lfw.at(carry + (int64_t)(ex >> 16));
        }
      }
      carry += (int64_t)(s_tot[buf] >> 16);
    }
    __syncthreads();  // (s_slot reused; s_w[buf] complete for the fold)
  }
  if (threadIdx.x == kWave) {  // (a scanner holds the observation count)
    if (carry != (int64_t)n && err) atomicOr(err, 4);
  }
  if (threadIdx.x == 0) cat_pseudocount(S, p, k, cnt);
}

// Long histories (n_rows >= kCathMinRows, at most kCathMaxCat categories):
// the single block per (segment, category) above walks every row itself --
// 13 windows of 7 680 rows at 100k rows, ~115 us of scanning alone (C5's
// categorical levels).  Chunked instead, the same bits:
//   k_cath_count  one block per (4096-row chunk, segment): the chunk's members
//                 and matches per category (ballots);
//   k_cath_emit   one block per (chunk, segment): every member's position in
//                 the segment (chunk base + wave base + rank in the tile) gives
//                 its LF weight, every match its place in its category's list,
//                 in row order -- the lists the single-block kernel folds;
//   k_cath_fold   one block of 8 waves per (segment, category): the list folded
//                 in order (block_fold_list: the serial chain's bits), staged
//                 through LDS 4 096 entries at a time.
constexpr int kCathMinRows = 32768;
constexpr int kCathMaxCat = 32;
constexpr int kCC = 4096;                 // rows per chunk
constexpr int kCathBS = 256;              // k_cath_count / k_cath_emit block
constexpr int kCathW = kCathBS / kWave;   // waves per chunk block
constexpr int kCathRPW = kCC / kCathW;    // rows per wave (1024)
constexpr int kCathT = kCathRPW / kWave;  // tiles of 64 rows per wave (16)
constexpr int kCathStride = 1 + kCathMaxCat;  // counts per (segment, chunk): members, matches

__host__ __device__ inline int64_t cath_chunks(int64_t n_rows) { return (n_rows + kCC - 1) / kCC; }
__host__ __device__ inline int64_t cath_count_bytes(int n_seg, int64_t n_rows) {
  return ((int64_t)4 * n_seg * cath_chunks(n_rows) * kCathStride + 255) & ~(int64_t)255;
}

// A chunk block's prologue, in two steps (as one helper k_cath_emit took 72
// VGPRs instead of 56): this wave's rows of the chunk loaded (cath_row's
// arguments; i0: this lane's first row, the others every 64) ...
__device__ __forceinline__ void cath_load(
    const double* __restrict__ V, const uint8_t* __restrict__ Ac,
    const int32_t* __restrict__ rows, const uint8_t* __restrict__ is_below, int64_t i0,
    int64_t n_rows, uint8_t side, int64_t offset, int K, bool (&mem)[kCathT],
    int (&cat)[kCathT]) {
#pragma unroll
  for (int t = 0; t < kCathT; ++t)
    cath_row(V, Ac, rows, is_below, i0 + t * kWave, n_rows, side, offset, K, mem[t], cat[t]);
}
// ... and counted by ballots: the wave's members in s_c[wave][0], its matches
// of category k in s_c[wave][1 + k]
__device__ __forceinline__ void cath_count(int K, const bool (&mem)[kCathT],
                                           const int (&cat)[kCathT],
                                           uint32_t (*s_c)[kCathStride]) {
  const int lane = lane_id(), w = threadIdx.x / kWave;
  uint32_t nm = 0;
#pragma unroll
  for (int t = 0; t < kCathT; ++t) nm += (uint32_t)__popcll(__ballot(mem[t]));
  if (lane == 0) s_c[w][0] = nm;
  for (int k = 0; k < K; ++k) {  // (block-uniform)
    uint32_t nk = 0;
#pragma unroll
    for (int t = 0; t < kCathT; ++t) nk += (uint32_t)__popcll(__ballot(cat[t] == k));
    if (lane == 0) s_c[w][1 + k] = nk;
  }
}

__global__ __launch_bounds__(kCathBS) void k_cath_count(
    const double* __restrict__ vals, const uint8_t* __restrict__ active, int64_t ld,
    const int32_t* __restrict__ rows, int64_t n_rows, const uint8_t* __restrict__ is_below,
    const tpe_gather* __restrict__ gathers, const tpe_cat_seg* __restrict__ segs,
    uint32_t* __restrict__ cnt) {
  __shared__ uint32_t s_c[kCathW][kCathStride];
  const int seg = blockIdx.y, c = blockIdx.x;
  const int K = segs[seg].n_cat;
  const tpe_gather G = gathers[seg];
  bool mem[kCathT];
  int cat[kCathT];
  const int64_t r0 = (int64_t)c * kCC + (int64_t)(threadIdx.x / kWave) * kCathRPW;
  cath_load(vals + (int64_t)G.col * ld, active + (int64_t)G.col * ld, rows, is_below,
            r0 + lane_id(), n_rows, G.below ? 1 : 0, G.offset, K, mem, cat);
  cath_count(K, mem, cat, s_c);
  __syncthreads();
  uint32_t* out = cnt + ((int64_t)seg * gridDim.x + c) * kCathStride;
  for (int j = threadIdx.x; j < 1 + K; j += kCathBS) {
    uint32_t v = 0;
#pragma unroll
    for (int q = 0; q < kCathW; ++q) v += s_c[q][j];
    out[j] = v;
  }
}

__global__ __launch_bounds__(kCathBS) void k_cath_emit(
    const double* __restrict__ vals, const uint8_t* __restrict__ active, int64_t ld,
    const int32_t* __restrict__ rows, int64_t n_rows, const uint8_t* __restrict__ is_below,
    const tpe_gather* __restrict__ gathers, const tpe_cat_seg* __restrict__ segs,
    const uint32_t* __restrict__ cnt, double* __restrict__ lists) {
  __shared__ uint32_t s_w[kCathW][kCathStride];   // per wave: members, matches
  __shared__ int64_t s_pre[kCathStride];          // chunks before this one
  __shared__ int64_t s_tot[kCathStride];          // the whole segment
  __shared__ int64_t s_cur[kCathW][kCathStride];  // per wave: next member position, list slots
  const int seg = blockIdx.y, c = blockIdx.x, nch = gridDim.x;
  const tpe_cat_seg S = segs[seg];
  const tpe_gather G = gathers[seg];
  const int lane = lane_id(), w = threadIdx.x / kWave;
  const uint64_t lt = (1ull << lane) - 1ull;
  const int K = S.n_cat;
  bool mem[kCathT];
  int cat[kCathT];
  const int64_t r0 = (int64_t)c * kCC + (int64_t)w * kCathRPW;
  cath_load(vals + (int64_t)G.col * ld, active + (int64_t)G.col * ld, rows, is_below, r0 + lane,
            n_rows, G.below ? 1 : 0, G.offset, K, mem, cat);
  cath_count(K, mem, cat, s_w);
  // the chunks before this one, and the segment's totals per category
  const uint32_t* C = cnt + (int64_t)seg * nch * kCathStride;
  for (int j = threadIdx.x; j < 1 + K; j += kCathBS) {
    int64_t pre = 0, tot = 0;
#pragma unroll 8
    for (int q = 0; q < nch; ++q) {  // (eight loads in flight)
      const int64_t v = C[(int64_t)q * kCathStride + j];
      pre += q < c ? v : 0;
      tot += v;
    }
    s_pre[j] = pre;
    s_tot[j] = tot;
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // per wave: its first member position and list slots
    int64_t m = s_pre[0];
    int64_t koff[kCathMaxCat];
    int64_t acc = (int64_t)seg * n_rows;  // (segment seg's lists start at seg * n_rows)
    for (int k = 0; k < K; ++k) {
      koff[k] = acc + s_pre[1 + k];
      acc += s_tot[1 + k];
    }
    for (int q = 0; q < kCathW; ++q) {
      s_cur[q][0] = m;
      m += s_w[q][0];
      for (int k = 0; k < K; ++k) {
        s_cur[q][1 + k] = koff[k];
        koff[k] += s_w[q][1 + k];
      }
    }
  }
  __syncthreads();
  // the wave's tiles in row order: member positions -> LF weights -> list slots
  const LfRamp lfw(S.n_obs, S.lf);
  int64_t mpos = s_cur[w][0];
#pragma unroll
  for (int t = 0; t < kCathT; ++t) {
    const uint64_t mb = __ballot(mem[t]);
    const int64_t pos = mpos + __popcll(mb & lt);
    mpos += __popcll(mb);
    int64_t slot = -1;
    for (int k = 0; k < K; ++k) {  // (block-uniform)
      const uint64_t kb = __ballot(cat[t] == k);
      if (kb == 0) continue;  // (wave-uniform)
      const int64_t base = s_cur[w][1 + k];
      if (cat[t] == k) slot = base + __popcll(kb & lt);
      if (lane == 0) s_cur[w][1 + k] = base + __popcll(kb);
      __builtin_amdgcn_wave_barrier();
    }
    if (slot >= 0) lists[slot] = lfw.at(pos);
  }
}

__global__ __launch_bounds__(kFB) void k_cath_fold(const tpe_cat_seg* __restrict__ segs,
                                                   const uint32_t* __restrict__ cnt, int nch,
                                                   int64_t n_rows,
                                                   const double* __restrict__ lists,
                                                   double* __restrict__ p,
                                                   int32_t* __restrict__ err) {
  __shared__ double s_l[kFoldN];
  __shared__ FoldX<kFW> X;
  __shared__ int64_t s_meta[3];
  const int seg = blockIdx.y, k = blockIdx.x;
  const tpe_cat_seg S = segs[seg];
  if (k >= S.n_cat) return;  // (block-uniform)
  const int lane = lane_id();
  const uint32_t* C = cnt + (int64_t)seg * nch * kCathStride;
  if (threadIdx.x < kWave) {  // this category's list: after the lists of categories < k
    int64_t before = 0, n_k = 0, members = 0;
    for (int q = lane; q < nch; q += kWave) {
      const uint32_t* Cq = C + (int64_t)q * kCathStride;
      for (int j = 0; j < k; ++j) before += Cq[1 + j];
      n_k += Cq[1 + k];
      members += Cq[0];
    }
    for (int o = 32; o >= 1; o >>= 1) {
      before += __shfl_xor(before, o, kWave);
      n_k += __shfl_xor(n_k, o, kWave);
      members += __shfl_xor(members, o, kWave);
    }
    if (lane == 0) {
      s_meta[0] = before;
      s_meta[1] = n_k;
      if (k == 0 && members != (int64_t)S.n_obs && err) atomicOr(err, 4);
    }
  }
  __syncthreads();
  const int64_t n_k = s_meta[1];
  const double* L = lists + (int64_t)seg * n_rows + s_meta[0];
  const double cntv = block_fold_list<kFSE, kFW>(0.0, L, n_k, 0, s_l, X);
  if (threadIdx.x == 0) cat_pseudocount(S, p, k, cntv);
}

// normalise (numpy pairwise sum), log p (categorical_lpdf, tpe.py:60-73) and
// the cumulative p of the inverse-CDF sampler; one block per segment
__global__ __launch_bounds__(kCatBS) void k_cat_finalize(const tpe_cat_seg* __restrict__ segs,
                                                         double* __restrict__ p,
                                                         double* __restrict__ logp,
                                                         double* __restrict__ cdf) {
  const tpe_cat_seg& S = segs[blockIdx.x];
  const int K = S.n_cat;
  __shared__ double total;
  if (threadIdx.x == 0) total = np_sum(p + S.p_off, K);
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += kCatBS) {
    const double pk = p[S.p_off + k] / total;
    p[S.p_off + k] = pk;
    logp[S.p_off + k] = log(pk);
  }
  __syncthreads();
  __shared__ double chunk_tot[kCatBS];
  const int per = (K + kCatBS - 1) / kCatBS;
  const int k0 = threadIdx.x * per, k1 = min(K, k0 + per);
  double run = 0.0;
  for (int k = k0; k < k1; ++k) {
    run += p[S.p_off + k];
    cdf[S.p_off + k] = run;
  }
  chunk_tot[threadIdx.x] = run;
  __syncthreads();
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (int t = 0; t < kCatBS; ++t) {
      const double c = chunk_tot[t];
      chunk_tot[t] = acc;
      acc += c;
    }
  }
  __syncthreads();
  const double base = chunk_tot[threadIdx.x];
  if (base != 0.0)
    for (int k = k0; k < k1; ++k) cdf[S.p_off + k] += base;
}
}  // namespace

}  // namespace tpe

using namespace tpe;

extern "C" int tpe_cat_posterior(const int64_t* obs, const tpe_cat_seg* segs, int n_seg,
                                 int max_cat, double* p_pool, double* logp_pool,
                                 double* cdf_pool, void* stream) {
  if (n_seg < 0 || (n_seg > 0 && (!segs || !p_pool || !logp_pool || !cdf_pool))) {
    set_error("tpe_cat_posterior: bad arguments");
    return TPE_E_ARG;
  }
  if (n_seg == 0) return TPE_OK;
  if (n_seg > 65535 || max_cat < 0) {
    set_error("tpe_cat_posterior: n_seg=%d max_cat=%d", n_seg, max_cat);
    return TPE_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const int gx = (std::max(max_cat, 1) + kCatWaves - 1) / kCatWaves;
  hipLaunchKernelGGL(k_cat_counts, dim3(gx, n_seg), dim3(kCatBS), 0, st, obs, segs, p_pool);
  hipLaunchKernelGGL(k_cat_finalize, dim3(n_seg), dim3(kCatBS), 0, st, segs, p_pool, logp_pool,
                     cdf_pool);
  return check_launch("tpe_cat_posterior");
}

extern "C" int64_t tpe_cat_hist_scratch_bytes(int n_seg, int max_cat, int64_t n_rows) {
  if (n_seg < 0 || max_cat < 0 || n_rows < 0) return -1;
  if (n_seg == 0 || n_rows < kCathMinRows || max_cat > kCathMaxCat) return 0;
  return cath_count_bytes(n_seg, n_rows) + (int64_t)8 * n_seg * n_rows;
}

extern "C" int tpe_cat_posterior_hist(const double* vals, const uint8_t* active, int64_t ld,
                                      const int32_t* rows, int64_t n_rows,
                                      const uint8_t* is_below, const tpe_gather* gathers,
                                      const tpe_cat_seg* segs, int n_seg, int max_cat,
                                      double* p_pool, double* logp_pool, double* cdf_pool,
                                      void* work, int64_t work_bytes, int32_t* err,
                                      void* stream) {
  if (n_seg < 0 || n_rows < 0 ||
      (n_seg > 0 && (!vals || !active || !is_below || !gathers || !segs || !p_pool ||
                     !logp_pool || !cdf_pool))) {
    set_error("tpe_cat_posterior_hist: bad arguments");
    return TPE_E_ARG;
  }
  if (n_seg == 0) return TPE_OK;
  if (n_seg > 65535 || max_cat < 0) {
    set_error("tpe_cat_posterior_hist: n_seg=%d max_cat=%d", n_seg, max_cat);
    return TPE_E_ARG;
  }
  if (work_bytes < 0) {
    set_error("tpe_cat_posterior_hist: work_bytes=%lld", (long long)work_bytes);
    return TPE_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const int64_t need = tpe_cat_hist_scratch_bytes(n_seg, max_cat, n_rows);
  if (need > 0 && work && work_bytes >= need && max_cat >= 1) {
    // a long history: chunked (k_cath_*); the same bits as k_cat_counts_hist
    const int64_t nch = cath_chunks(n_rows);
    if (nch > INT32_MAX) {
      set_error("tpe_cat_posterior_hist: n_rows=%lld", (long long)n_rows);
      return TPE_E_UNSUPPORTED;
    }
    uint32_t* cnt = static_cast<uint32_t*>(work);
    double* lists = reinterpret_cast<double*>(static_cast<char*>(work) +
                                              cath_count_bytes(n_seg, n_rows));
    const dim3 g((unsigned)nch, n_seg);
    hipLaunchKernelGGL(k_cath_count, g, dim3(kCathBS), 0, st, vals, active, ld, rows, n_rows,
                       is_below, gathers, segs, cnt);
    hipLaunchKernelGGL(k_cath_emit, g, dim3(kCathBS), 0, st, vals, active, ld, rows, n_rows,
                       is_below, gathers, segs, cnt, lists);
    hipLaunchKernelGGL(k_cath_fold, dim3(max_cat, n_seg), dim3(kFB), 0, st, segs, cnt,
                       (int)nch, n_rows, lists, p_pool, err);
  } else {
    hipLaunchKernelGGL(k_cat_counts_hist, dim3(std::max(max_cat, 1), n_seg), dim3(kCHB), 0, st,
                       vals, active, ld, rows, n_rows, is_below, gathers, segs, p_pool, err);
  }
  hipLaunchKernelGGL(k_cat_finalize, dim3(n_seg), dim3(kCatBS), 0, st, segs, p_pool, logp_pool,
                     cdf_pool);
  return check_launch("tpe_cat_posterior_hist");
}
