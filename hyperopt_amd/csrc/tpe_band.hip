// tpe_band.hip -- the band rescue of the fast table scorer: the candidates
// whose fp32 score bound reaches the best lower bound (the band tiles
// k_score_table_fast writes, tpe_table.hpp) are re-scored in fp64 with
// GMM1_lpdf / LGMM1_lpdf's sums (hyperopt/tpe.py:117-180, 265-307), and
// broadcast_best's argmax (tpe.py:649-658) is taken over them.
//
// Exports: tpe_band_bytes, tpe_band_rescore, tpe_band_layout; launch_reduce
// (k_reduce) for every scorer.
#include <cstddef>

#include "tpe_table.hpp"

namespace tpe {
namespace {
// ---------------------------------------------------------------------------
// exact re-score of the band: one kernel (k_band), kBandBlocks blocks per job
// ---------------------------------------------------------------------------
// Every survivor's two log-densities are summed in fp64 over EVERY component
// (within e^-45 of the sum) -- GMM1_lpdf / LGMM1_lpdf's sums (tpe.py:117-180,
// 265-307; LGMM1's -log x cancels in the score) -- and its score is a
// function of its y alone, whatever the sharding of the candidates, within
// fp64 rounding of the reference's.  Two ways, per job:
//  * few survivors (<= kBandSurv; a peaked score): directly -- the components
//    split into kBandBlocks chunks, one block each, every survivor's partial
//    log-sum-exp per chunk (per thread an online sum in a fixed order, then a
//    fixed reduction tree), the chunks combined in order by the job's last
//    block;
//  * many (a flat score: thousands within the band, in a few cells): per
//    table cell holding survivors, both mixtures expanded around the cell
//    centre to degree kBandD (band_expand; components whose series would
//    converge slowly summed term by term), the cells dealt to the job's
//    blocks; survivors off the grid or past the kBandCells listed take the
//    direct sum (band_direct).
// Steps of every block:
//  1. G = max over the job's tiles of their lo; a tile whose entries did not
//     fit (kTileFull) with hi_max >= G makes the job "overflowed": block 0
//     gives the fp32 winner with n_scored = -1 (the caller re-scores the job
//     exactly).
//  2. The survivors -- entries with hi >= G of the tiles with hi_max >= G, in
//     flat entry order, the same in every block.  The exact winner i* is
//     among them: lo_k <= s64_k <= s64_i* <= hi_i* for every k, so hi_i* >=
//     G, and i* is in its tile's entries (hi_i* >= G >= that tile's lo);
//     every other candidate has s64 <= hi < G <= s64_i*.
//  3. The block's share of the sums (above).
//  4. The last block of the job to finish takes np.argmax over the
//     survivors (largest score, then smallest index, NaN first): best[j] =
//     {fp64 score, index, value, n_cand}, and re-arms the counter.
#ifndef TPE_BAND_BLOCKS  // diagnostic builds: k_band blocks per job
#define TPE_BAND_BLOCKS 16
#endif
constexpr int kBandBlocks = TPE_BAND_BLOCKS;  // blocks per job
constexpr int kBandSurv = 128;       // survivors a job may score directly
#ifndef TPE_BAND_DIRECT
#define TPE_BAND_DIRECT 128
#endif
constexpr int kBandDirect = TPE_BAND_DIRECT;  // ... and always does; more take the cell
                                              // expansions where the cells can hold them.
// (16 made drop-in bands of 30-130 survivors cheaper, but a rank's share of
// a label can then take the other path than the whole label and score the
// same candidate with other fp64 bits: the winners must not depend on the
// rank count -- test_gpu_shard.py -- so a job's path keeps to 128.)
#ifndef TPE_SURV_BATCH
#define TPE_SURV_BATCH 8
#endif
constexpr int kSurvBatch = TPE_SURV_BATCH;  // survivors summed together per pass
constexpr int kDirStage = 256;       // a block's component chunk staged in LDS when it fits
                                     // (a multiple of kBX: the per-thread order is unchanged;
                                     // small: k_band shares CUs with the side stream's launches)
#ifndef TPE_BAND_BX
#define TPE_BAND_BX 256
#endif
constexpr int kBX = TPE_BAND_BX;     // k_band block
constexpr int kBandTiles = 4096;     // tiles of a job the kernel's LDS prefix holds (2^24 candidates;
                                     // a larger job takes the exact fallback)
constexpr int kTilesPT = kBandTiles / kBX;  // tile headers per thread (prefix pass)
constexpr int kBandD = 20;           // expansion degree
constexpr double kBandTau = 45.0;    // exclusion margin (nats) on top of log(M)
constexpr double kBandRho = 1.5;     // admissible 1.05 |A| + 1.1025 |B|
constexpr int kBandCells = 64;       // cells expanded per job (sorted; the rest: direct)
constexpr int kBandBits = 32768;     // cell bitmap (LDS)

#ifndef TPE_BAND_DIR
#define TPE_BAND_DIR 16
#endif
constexpr int kChunkDir = TPE_BAND_DIR;  // slow components listed per (cell, chunk, mixture)
                                          // (a full list sends the cell's survivors to the
                                          // direct sum over every component)
struct BandMix {  // one mixture's expansion on one cell (or one chunk of its components)
  double P[kBandD + 1];
  double m;
  int n_dir;  // slow components listed; -1: more than fit (the job takes the exact fallback)
  int pad;
  int dir[kChunkDir];
};
#ifndef TPE_BAND_EPT
#define TPE_BAND_EPT 8
#endif
#ifndef TPE_BAND_U
#define TPE_BAND_U 2
#endif
constexpr int kEPT = TPE_BAND_EPT;   // band entries per thread per window (k_band)
constexpr int kExpU = TPE_BAND_U;    // band_expand: component loads in flight per thread
constexpr int kBandSurvMax = 65536;  // survivors a job may have (more: the exact fallback)
struct BandWork {  // per job (tpe_band_bytes)
  double part[kBandBlocks][kBandSurv][4];         // direct: per chunk and survivor {m, s} b, a
  BandMix cpart[kBandCells][kBandBlocks][2];      // cells: per cell, chunk and mixture
  float sy[kBandSurvMax];                         // the survivors (flat entry order): y ...
  int64_t sidx[kBandSurvMax];                     // ... and candidate index
  int cells[kBandCells];                          // the listed cells (ascending)
  int ns, ncell, over, direct;                    // survivors, cells, job overflowed, path
  long long tmark[16];                            // (TPE_BAND_TIMING diagnostic builds)
  BestT win[kBandBlocks];                         // k_band_final's per-block winners (k_band_pick)
  unsigned int done;                              // (unused)
  unsigned int pad[3];
};

// One step of the online log-sum-exp (s >= 1 at scale m) that needs no exp
// and changes nothing in the result's bits: a term below e^-37 of the
// scale adds < 2^-53 <= ulp(s)/2 to s (s is left as it is, as the rounded
// add would); a term above e^60 of it makes s * e^(m - v) < 2^-53 for any
// s < 1e10 (s = 1 + that rounds to 1).  NaN differences fall through.
__device__ __forceinline__ bool lse_skip(double& m, double& s, double v) {
  const double d = v - m;
  if (d < -37.0) return true;
  if (d > 60.0) {
    s = 1.0;
    m = v;
    return true;
  }
  return false;
}

// (m, s): e^m s; combined in a fixed order
__device__ __forceinline__ void lse_merge(double& m, double& s, double m2, double s2) {
  if (m2 == -INFINITY) return;
  if (m2 > m) {
    s = s * exp(m - m2) + s2;
    m = m2;
  } else {
    s += s2 * exp(m2 - m);
  }
}

// expansion of mixture S on the cell (y0, h) into E (LDS); all threads.
// One pass over the components, U loads in flight per thread; each thread
// keeps its own scale (raised when a term would exceed e^8 of it) and the
// threads are merged at the end (fixed order: deterministic).  A component's
// series exp(A u + B u^2) converges like rho^n / n!, rho = 1.05|A| +
// 1.1025|B|: with rho <= kBandRho the tail past degree 20 is < 1.1e-16 of
// its term (1.5^21 / 21!; a component the table admitted has rho <= 0.68:
// < 4e-23); components with a larger rho are summed term by term.
// Components whose largest term on the cell is below e^-45 / M of the prior
// component's smallest one there are left out (< e^-45 of the sum).
template <int BX, int U>
__device__ void band_expand(const tpe_seg& S, const double* __restrict__ coef64, double y0,
                            double h, BandMix& E, double* dred, int k_begin, int k_end) {
  const int nc = S.n_obs + 1;  // (the floor is the whole mixture's)
  const int64_t off = S.comp_off;
  const double4 cp = ld4(coef64, off + S.prior_pos);
  const double far = (fabs(y0 - cp.x) + 1.05 * h) * cp.y;
  const double T = cp.z - 0.5 * far * far - (log((double)nc) + kBandTau);
  if (threadIdx.x == 0) E.n_dir = 0;
  __syncthreads();
  double P[kBandD + 1];
#pragma unroll
  for (int n = 0; n <= kBandD; ++n) P[n] = 0.0;
  double ml = -INFINITY;
  for (int k0 = k_begin; k0 < k_end; k0 += U * BX) {
    double4 cs[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = k0 + u * BX + (int)threadIdx.x;
      cs[u] = k < k_end ? ld4(coef64, off + k) : make_double4(0.0, 0.0, -INFINITY, 0.0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const double4 c = cs[u];
      const double zn = fmax(fabs(y0 - c.x) - 1.05 * h, 0.0) * c.y;
      if (!(c.z - 0.5 * zn * zn >= T)) continue;  // (padding: lc = -inf)
      const double hi2 = h * c.y * c.y;
      const double A = -(y0 - c.x) * hi2, B = -0.5 * h * hi2;
      if (1.05 * fabs(A) + 1.1025 * fabs(B) > kBandRho) {
        const int p = atomicAdd(&E.n_dir, 1);
        if (p < kChunkDir) E.dir[p] = k0 + u * BX + (int)threadIdx.x;
        continue;
      }
      const double z0 = (y0 - c.x) * c.y;
      const double v = c.z - 0.5 * z0 * z0;
      if (v > ml + 8.0) {  // new scale: rescale this thread's sums
        const double r = (ml == -INFINITY) ? 0.0 : exp(ml - v);
#pragma unroll
        for (int n = 0; n <= kBandD; ++n) P[n] *= r;
        ml = v;
      }
      double cm = 0.0, cc = exp(v - ml);  // e * c_n
      P[0] += cc;
#pragma unroll
      for (int n = 0; n < kBandD; ++n) {
        const double cn = fma(A, cc, 2.0 * B * cm) * (1.0 / (double)(n + 1));
        P[n + 1] += cn;
        cm = cc;
        cc = cn;
      }
    }
  }
  const double m = block_max<BX, double>(ml, dred);
  {
    const double r = (ml == -INFINITY) ? 0.0 : exp(ml - m);
#pragma unroll
    for (int n = 0; n <= kBandD; ++n) P[n] *= r;
  }
  // block sums of the kBandD + 1 terms (fixed order: deterministic)
  // (every term's butterfly stepped together: their LDS exchanges overlap)
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    double t[kBandD + 1];
#pragma unroll
    for (int n = 0; n <= kBandD; ++n) t[n] = __shfl_xor(P[n], o, kWave);
#pragma unroll
    for (int n = 0; n <= kBandD; ++n) P[n] += t[n];
  }
  __syncthreads();  // (E.n_dir complete; dred free)
  const int wid = threadIdx.x / kWave;
  if (lane_id() == 0) {
#pragma unroll
    for (int n = 0; n <= kBandD; ++n) dred[wid * (kBandD + 1) + n] = P[n];
  }
  __syncthreads();
  if (threadIdx.x <= kBandD) {
    double t = 0.0;
    for (int w = 0; w < BX / kWave; ++w) t += dred[w * (kBandD + 1) + threadIdx.x];
    E.P[threadIdx.x] = t;
  }
  if (threadIdx.x == 0) {
    E.m = m;
    if (E.n_dir > kChunkDir) E.n_dir = -1;
  }
  __syncthreads();
}

// log of the mixture at y summed directly over every component (online
// log-sum-exp, k_score64's arithmetic)
__device__ __forceinline__ double band_direct(const tpe_seg& S, const double* __restrict__ coef64,
                                              double y) {
  double mo = -INFINITY, so = 0.0;
  for (int k = 0; k < S.n_obs + 1; ++k) {
    const double4 c = ld4(coef64, S.comp_off + k);
    const double t = (y - c.x) * c.y;
    const double v = -0.5 * (t * t) + c.z;
    if (lse_skip(mo, so, v)) continue;
    const bool up = v > mo;
    const double e = exp(up ? mo - v : v - mo);
    so = up ? so * e + 1.0 : so + e;
    mo = up ? v : mo;
  }
  return log(so) + mo;
}

// the fp32 cell of a band candidate (as the scorer forms it); -2: off the
// grid (the direct sum)
__device__ __forceinline__ int band_cell(const tpe_table& Tb, float y) {
  const float g0 = (float)Tb.origin, h32 = (float)Tb.h;
  const float t = (y - g0) * Tb.inv_w;
  int c = (t >= 0.0f) ? (int)t : 0;
  c = min(c, Tb.nb - 1);
  const double u = ((double)y - (double)cell_centre(g0, h32, c)) / Tb.h;
  return (fabs(u) <= (double)kULim && y == y) ? c : -2;
}

__global__ __launch_bounds__(kBX) void k_band(
    const tpe_job* __restrict__ jobs, const tpe_seg* __restrict__ segs,
    const double* __restrict__ coef64, const tpe_table* __restrict__ tables,
    const tpe_band* __restrict__ band, const uint32_t* __restrict__ band_ctl,
    const tpe_best* __restrict__ partial, int n_tiles, tpe_best* __restrict__ best,
    BandWork* __restrict__ work) {
  constexpr int kNW = kBX / kWave;
  __shared__ BestT red[kNW];
  __shared__ int s_end[kBandTiles];  // inclusive prefix of the tiles' counted entries
  __shared__ uint32_t s_bits[kBandBits / 32];
  __shared__ int s_cell[kBandCells];
  __shared__ float s_y[kBandSurv];
  __shared__ int64_t s_idx[kBandSurv];
  __shared__ int s_wt[kNW];
  __shared__ float s_g[kNW];
  __shared__ double s_red[kNW][kSurvBatch][2];
  __shared__ double dred[kNW * (kBandD + 1)];
  __shared__ BandMix s_eb;
  __shared__ int s_over, s_off;
  __shared__ int s_tile[kEPT * kBX];
  __shared__ int s_wm[kNW];
  __shared__ double4 s_cst[kDirStage];  // direct path: the block's chunk of one mixture
  const int j = blockIdx.y, kb = blockIdx.x;
  const int lane = lane_id(), wid = threadIdx.x / kWave;
  const tpe_job J = jobs[j];
  const uint32_t* H = band_ctl + (int64_t)j * n_tiles * kHdrWords;
  const tpe_band* Bj = band + (int64_t)j * n_tiles * kTileSlots;
  // exclusive block scan of one int per thread (wave scan + wave totals)
  auto block_excl = [&](int v, int& total) -> int {
    int incl = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int w = __shfl_up(incl, o, kWave);
      if (lane >= o) incl += w;
    }
    __syncthreads();
    if (lane == kWave - 1) s_wt[wid] = incl;
    __syncthreads();
    int pos = incl - v;
    total = 0;
#pragma unroll
    for (int w = 0; w < kNW; ++w) {
      pos += w < wid ? s_wt[w] : 0;
      total += s_wt[w];
    }
    return pos;
  };
#ifdef TPE_BAND_TIMING
#define TMARK(i) \
  if (blockIdx.x == 0 && threadIdx.x == 0) work[blockIdx.y].tmark[i] = wall_clock64();
#else
#define TMARK(i)
#endif
  TMARK(0)
  // ---- 1. G, overflow, the tiles' counts ----
  float g = -INFINITY;
  for (int t = threadIdx.x; t < n_tiles; t += kBX) g = fmaxf(g, __uint_as_float(H[t * kHdrWords]));
  g = wave_max_f(g);
  if (lane == 0) s_g[wid] = g;
  if (threadIdx.x == 0) s_over = n_tiles > kBandTiles;
  for (int w = threadIdx.x; w < kBandBits / 32; w += kBX) s_bits[w] = 0u;
  __syncthreads();
  float G = s_g[0];
#pragma unroll
  for (int w = 1; w < kNW; ++w) G = fmaxf(G, s_g[w]);
  // the relevant tiles' counts in LDS, then their inclusive prefix in place
  for (int t = threadIdx.x; t < kBandTiles; t += kBX) {
    int c = 0;
    if (t < n_tiles) {
      const float hm = __uint_as_float(H[t * kHdrWords + 1]);
      const uint32_t n = H[t * kHdrWords + 2];
      if (!(hm < G) && n != 0u) {
        if (n == kTileFull) s_over = 1;
        else c = (int)n;
      }
    }
    s_end[t] = c;
  }
  __syncthreads();
  int tot = 0;
  for (int i = 0; i < kTilesPT; ++i) tot += s_end[threadIdx.x * kTilesPT + i];
  int n_ent = 0;
  int run = block_excl(tot, n_ent);
  for (int i = 0; i < kTilesPT; ++i) {
    run += s_end[threadIdx.x * kTilesPT + i];
    s_end[threadIdx.x * kTilesPT + i] = run;
  }
  __syncthreads();
  if (s_over) {  // the fp32 winner; the caller re-scores the job exactly
    if (kb == 0) {
      BestT b32 = thread_best<kBX>(partial + (int64_t)j * n_tiles, n_tiles);
      b32 = block_best<kBX>(b32, red);
      if (threadIdx.x == 0) {
        best[j] = tpe_best{b32.score, b32.index, b32.value, -1};
        work[j].over = 1;  // (k_band_final / k_band_pick leave the job alone)
      }
    }
    return;
  }
  const int nt = min(n_tiles, kBandTiles);
  const tpe_table Tb = tables[j];
  // every entry once, kEPT consecutive ones per thread loaded together;
  // fn(entry, flat position) for the survivors, every thread taking part.
  // A window's flat positions find their tile without a search: each tile
  // marks its first position in the window with its id, and a running max
  // over the window (thread, then wave and block prefix) fills the rest.
  constexpr int kWin = kEPT * kBX;
  auto for_survivors = [&](auto&& fn) {
    for (int f0 = 0; f0 < n_ent; f0 += kWin) {
      for (int i = threadIdx.x; i < kWin; i += kBX) s_tile[i] = -1;
      __syncthreads();
      for (int t = threadIdx.x; t < nt; t += kBX) {
        const int st = t > 0 ? s_end[t - 1] : 0, en = s_end[t];
        if (en > st && en > f0 && st < f0 + kWin) s_tile[max(st, f0) - f0] = t;
      }
      __syncthreads();
      int tl[kEPT];
      int run = -1;
#pragma unroll
      for (int u = 0; u < kEPT; ++u) {
        run = max(run, s_tile[threadIdx.x * kEPT + u]);
        tl[u] = run;
      }
      int incl = run;  // inclusive max-scan over the wave, then the waves before
#pragma unroll
      for (int o = 1; o < kWave; o <<= 1) {
        const int w = __shfl_up(incl, o, kWave);
        if (lane >= o) incl = max(incl, w);
      }
      int carry = __shfl_up(incl, 1, kWave);
      if (lane == 0) carry = -1;
      if (lane == kWave - 1) s_wm[wid] = incl;
      __syncthreads();
#pragma unroll
      for (int w = 0; w < kNW; ++w) carry = w < wid ? max(carry, s_wm[w]) : carry;
      tpe_band E[kEPT];
#pragma unroll
      for (int u = 0; u < kEPT; ++u) {
        const int f = f0 + threadIdx.x * kEPT + u;
        E[u].hi = -INFINITY;
        if (f < n_ent) {
          const int t = max(tl[u], carry);
          const int e = f - (t > 0 ? s_end[t - 1] : 0);
          E[u] = Bj[(int64_t)t * kTileSlots + e];
        }
      }
      uint32_t keep = 0;
#pragma unroll
      for (int u = 0; u < kEPT; ++u)
        if (f0 + threadIdx.x * kEPT + u < n_ent && !(E[u].hi < G)) keep |= 1u << u;
      fn(E, keep);
    }
  };
  TMARK(1)
  // ---- 2. the survivors: their number and cells; block 0 lists them (flat
  // entry order) for k_band_final ----
  BandWork& W = work[j];
  int ns = 0;
  if (threadIdx.x == 0) s_off = 0;
  for_survivors([&](const tpe_band (&E)[kEPT], uint32_t keep) {
    int total = 0;
    int pos = ns + block_excl(__popc(keep), total);
#pragma unroll
    for (int u = 0; u < kEPT; ++u) {
      if ((keep >> u) & 1u) {
        if (pos < kBandSurv) {
          s_y[pos] = E[u].y;
          s_idx[pos] = E[u].index;
        }
        if (kb == 0 && pos < kBandSurvMax) {
          W.sy[pos] = E[u].y;
          W.sidx[pos] = E[u].index;
        }
        ++pos;
        const int c = band_cell(Tb, E[u].y);
        // (read first: a band's thousands of survivors share a few cells,
        // and same-word LDS atomics serialise)
        if (c >= 0 && c < kBandBits) {
          if (!(s_bits[c >> 5] & (1u << (c & 31)))) atomicOr(&s_bits[c >> 5], 1u << (c & 31));
        } else {
          s_off = 1;
        }
      }
    }
    ns += total;
  });
  __syncthreads();
  // the listed cells (ascending)
  constexpr int kPer = kBandBits / 32 / kBX;  // bitmap words per thread
  int ncell = 0;
  {
    int c = 0;
#pragma unroll
    for (int i = 0; i < kPer; ++i) c += __popc(s_bits[threadIdx.x * kPer + i]);
    int pos = block_excl(c, ncell);
    for (int i = 0; i < kPer && pos < kBandCells; ++i) {
      uint32_t b = s_bits[threadIdx.x * kPer + i];
      while (b && pos < kBandCells) {
        const int cell = (threadIdx.x * kPer + i) * 32 + __builtin_ctz(b);
        s_cell[pos] = cell;
        if (kb == 0) W.cells[pos] = cell;
        ++pos;
        b &= b - 1;
      }
    }
  }
  __syncthreads();
  TMARK(2)
  // the path: a few survivors are summed directly; more take the cell
  // expansions (their cost does not grow with the survivors: ~12 us against
  // ~5 us per 8 direct survivors), up to kBandSurv directly when the cells
  // cannot hold them (too many, or survivors off the grid); else the exact
  // fallback
  const bool cells_ok = ncell <= kBandCells && !s_off && ns <= kBandSurvMax;
  const bool direct = ns <= kBandDirect || (ns <= kBandSurv && !cells_ok);
  const bool over = !direct && !cells_ok;
  if (kb == 0 && threadIdx.x == 0) {
    W.ns = ns;
    W.ncell = min(ncell, kBandCells);
    W.over = over;
    W.direct = direct;
  }
  if (over) {
    // many survivors, off the grid or over too many cells: the exact fallback
    if (kb == 0) {
      BestT b32 = thread_best<kBX>(partial + (int64_t)j * n_tiles, n_tiles);
      b32 = block_best<kBX>(b32, red);
      if (threadIdx.x == 0) best[j] = tpe_best{b32.score, b32.index, b32.value, -1};
    }
    return;
  }
  const tpe_seg SB = segs[J.below], SA = segs[J.above];
  const bool lgmm = J.family == TPE_LGMM1;
  if (direct) {
    // ---- 3a. direct: this block's component chunk, for every survivor ----
    for (int mix = 0; mix < 2; ++mix) {
      const tpe_seg& S = mix ? SA : SB;
      const int nc = S.n_obs + 1;
      const int per = (nc + kBandBlocks - 1) / kBandBlocks;
      const int k0 = kb * per, k1 = min(nc, k0 + per);
      const double4* C = reinterpret_cast<const double4*>(coef64) + S.comp_off;
      // the chunk in LDS once (every batch of survivors re-reads it; each
      // thread's components and their order are the global loop's)
      const bool staged = k1 - k0 <= kDirStage;
      if (staged) {
        for (int k = k0 + (int)threadIdx.x; k < k1; k += kBX) s_cst[k - k0] = C[k];
        __syncthreads();
      }
      TMARK(8 + 3 * mix)
      for (int b0 = 0; b0 < ns; b0 += kSurvBatch) {
        const int nbat = min(kSurvBatch, ns - b0);  // (block-uniform: the batch's real survivors)
        double m[kSurvBatch], sm[kSurvBatch], y[kSurvBatch];
#pragma unroll
        for (int i = 0; i < kSurvBatch; ++i) {
          m[i] = -INFINITY;
          sm[i] = 0.0;
          y[i] = score_coord(s_y[min(b0 + i, ns - 1)], lgmm);
        }
        auto acc = [&](const double4 c) {
#pragma unroll
          for (int i = 0; i < kSurvBatch; ++i) {
            if (i >= nbat) continue;  // (a short batch: no work for its empty slots)
            const double t = (y[i] - c.x) * c.y;
            const double v = -0.5 * (t * t) + c.z;  // (log coefficient c.z: GMM1_lpdf's terms)
            if (lse_skip(m[i], sm[i], v)) continue;
            const bool upv = v > m[i];
            const double e = exp(upv ? m[i] - v : v - m[i]);
            sm[i] = upv ? sm[i] * e + 1.0 : sm[i] + e;
            m[i] = upv ? v : m[i];
          }
        };
        if (staged) {
          for (int k = k0 + (int)threadIdx.x; k < k1; k += kBX) acc(s_cst[k - k0]);
        } else {
          for (int k = k0 + (int)threadIdx.x; k < k1; k += kBX) acc(C[k]);
        }
        if (b0 == 0) { TMARK(9 + 3 * mix) }
        // fixed reduction tree: the wave's largest scale (DPP max), each lane's
        // sum brought to it once, a plain wave sum; then the block's waves in
        // order (lse_merge)
        // (plain max and sum butterflies, the batch's survivors stepped
        // together so their LDS exchanges overlap: same bits)
        double mw[kSurvBatch], v[kSurvBatch];
#pragma unroll
        for (int i = 0; i < kSurvBatch; ++i) mw[i] = m[i];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
          double t[kSurvBatch];
#pragma unroll
          for (int i = 0; i < kSurvBatch; ++i) t[i] = __shfl_xor(mw[i], off, kWave);
#pragma unroll
          for (int i = 0; i < kSurvBatch; ++i) mw[i] = fmax(mw[i], t[i]);
        }
#pragma unroll
        for (int i = 0; i < kSurvBatch; ++i)
          v[i] = (m[i] == -INFINITY) ? 0.0 : sm[i] * exp(m[i] - mw[i]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
          double t[kSurvBatch];
#pragma unroll
          for (int i = 0; i < kSurvBatch; ++i) t[i] = __shfl_xor(v[i], off, kWave);
#pragma unroll
          for (int i = 0; i < kSurvBatch; ++i) v[i] += t[i];
        }
        if (lane == 0) {
#pragma unroll
          for (int i = 0; i < kSurvBatch; ++i) {
            s_red[wid][i][0] = mw[i];
            s_red[wid][i][1] = v[i];
          }
        }
        __syncthreads();
        if (threadIdx.x < kSurvBatch && b0 + (int)threadIdx.x < ns) {
          const int i = threadIdx.x;
          double mm = s_red[0][i][0], ss = s_red[0][i][1];
          for (int w = 1; w < kNW; ++w) lse_merge(mm, ss, s_red[w][i][0], s_red[w][i][1]);
          W.part[kb][b0 + i][2 * mix] = mm;
          W.part[kb][b0 + i][2 * mix + 1] = ss;
        }
        __syncthreads();  // (s_red reused; s_cst free after the last batch)
        if (b0 == 0) { TMARK(10 + 3 * mix) }
      }
    }
  } else {
    // ---- 3b. cells: (cell, chunk) units, kBandBlocks of them when the cells
    // are fewer (each cell's components in nch chunks), else one cell each;
    // block kb takes units kb, kb + kBandBlocks, ... (k_band_final merges
    // a cell's chunks in order) ----
    const float g0 = (float)Tb.origin, h32 = (float)Tb.h;
    const int nch = max(1, kBandBlocks / max(ncell, 1));
    for (int unit = kb; unit < ncell * nch; unit += kBandBlocks) {
      const int k = unit / nch, ch = unit % nch;
      const double y0 = (double)cell_centre(g0, h32, s_cell[k]);
      for (int mix = 0; mix < 2; ++mix) {
        const tpe_seg& S = mix ? SA : SB;
        const int nc = S.n_obs + 1;
        const int per = (nc + nch - 1) / nch;
        const int k0 = min(nc, ch * per), k1 = min(nc, k0 + per);
        band_expand<kBX, kExpU>(S, coef64, y0, Tb.h, s_eb, dred, k0, k1);
        BandMix& Q = W.cpart[k][ch][mix];
        if (threadIdx.x <= kBandD) Q.P[threadIdx.x] = s_eb.P[threadIdx.x];
        if (threadIdx.x == 0) {
          Q.m = s_eb.m;
          Q.n_dir = s_eb.n_dir;
        }
        if (threadIdx.x < kChunkDir) Q.dir[threadIdx.x] = s_eb.dir[threadIdx.x];
        __syncthreads();  // (s_eb reused)
      }
    }
  }
  TMARK(3)
}

// The band's decision (after k_band), kFinBlocks blocks per job, each
// scoring a share of the job's survivors: direct -- a survivor's kBandBlocks
// chunk partial sums merged on 16 lanes (the largest scale by a max
// butterfly, the chunks' sums brought to it and added by a fixed butterfly);
// cells -- each listed cell's chunk expansions merged in chunk order (into
// LDS; every block the same) and evaluated at the block's survivors.  Each
// block leaves its np.argmax in W.win[kb]; k_band_pick folds them into
// best[j] = {fp64 score, index, value, n_cand}.  (One block per job scored a
// C3 band of ~4 000 survivors in ~16 us on one CU: fp64-rate bound; a
// last-block hand-off inside the kernel cost 10-17 us in round 3.)
#ifndef TPE_BAND_FX
#define TPE_BAND_FX 512
#endif
#ifndef TPE_BAND_FINB
#define TPE_BAND_FINB 8
#endif
constexpr int kFX = TPE_BAND_FX;         // k_band_final block
constexpr int kFinBlocks = TPE_BAND_FINB;  // k_band_final blocks per job (<= kBandBlocks: W.win)
constexpr int kFStage = 512;   // survivors staged in LDS per round (k_band_final, cells; small:
                               // the kernel shares CUs with the side stream's big launches)
static_assert(kFinBlocks <= kBandBlocks && kFinBlocks <= kWave, "W.win holds the blocks' winners");
__global__ __launch_bounds__(kFX) void k_band_final(const tpe_job* __restrict__ jobs,
                                                    const tpe_seg* __restrict__ segs,
                                                    const double* __restrict__ coef64,
                                                    const tpe_table* __restrict__ tables,
                                                    BandWork* __restrict__ work) {
  constexpr int kNW = kFX / kWave;
  __shared__ BestT red[kNW];
  __shared__ double s_P[kBandCells][2][kBandD + 2];  // merged expansions: P_0..P_20, m
  __shared__ double s_tmp[kBandCells][2][kBandD + 2];  // per (cell, chunk) unit: its P and m
  __shared__ int s_nd[kBandCells][2];
  __shared__ int s_ndu[kBandCells][2];             // per (cell, chunk) unit: slow components ...
  __shared__ int s_dir[kBandCells][2][kChunkDir];  // ... and their indices (units <= kBandCells)
  __shared__ int s_cells[kBandCells];
  __shared__ float s_sy[kFStage];
  __shared__ int64_t s_si[kFStage];
  const int j = blockIdx.y, kb = blockIdx.x;
  BandWork& W = work[j];
  if (kb == 0) { TMARK(4) }
  if (W.over) return;  // (k_band gave the fp32 winner with n_scored = -1)
  const tpe_job J = jobs[j];
  const int ns = W.ns, ncell = W.ncell;
  const int nch = max(1, kBandBlocks / max(ncell, 1));  // (k_band's chunks per cell)
  const bool lgmm = J.family == TPE_LGMM1;
  const tpe_seg SB = segs[J.below], SA = segs[J.above];
  const tpe_table Tb = tables[j];
  BestT bx{0.0, -1, 0.0};
  if (W.direct) {
    // one survivor per 16 lanes, lane c holding chunk c's partials
    constexpr int kSPB = kFX / kBandBlocks;  // survivors per block pass
    static_assert(kBandBlocks == 16, "16-lane groups");
    const int c = threadIdx.x % kBandBlocks;
    for (int i = kb * kSPB + (int)threadIdx.x / kBandBlocks; i < ns; i += kFinBlocks * kSPB) {
      const double4 q = *reinterpret_cast<const double4*>(W.part[c][i]);
      double mb = q.x, ma = q.z;
#pragma unroll
      for (int o = kBandBlocks / 2; o >= 1; o >>= 1) {
        const double tb = __shfl_xor(mb, o, kWave), ta = __shfl_xor(ma, o, kWave);
        mb = fmax(mb, tb);
        ma = fmax(ma, ta);
      }
      double sb = q.x == -INFINITY ? 0.0 : q.y * exp(q.x - mb);
      double sa = q.z == -INFINITY ? 0.0 : q.w * exp(q.z - ma);
#pragma unroll
      for (int o = kBandBlocks / 2; o >= 1; o >>= 1) {
        const double tb = __shfl_xor(sb, o, kWave), ta = __shfl_xor(sa, o, kWave);
        sb += tb;
        sa += ta;
      }
      if (c == 0) best_update(bx, (log(sb) + mb) - (log(sa) + ma), W.sidx[i],
                              cand_value(W.sy[i], lgmm));
    }
  } else {
    // merge: the chunks' expansions (P_0..P_20 and m per (cell, chunk,
    // mixture)) staged in LDS with all their global reads in flight at once,
    // then thread t takes (cell, mixture, term) items: every term summed over
    // the chunks in order at the cell's largest scale
    for (int t = threadIdx.x; t < ncell * nch * 2 * (kBandD + 2); t += kFX) {
      const int n = t % (kBandD + 2), r = t / (kBandD + 2), u = r >> 1, mix = r & 1;
      const BandMix& q = W.cpart[u / nch][u % nch][mix];
      s_tmp[u][mix][n] = n <= kBandD ? q.P[n] : q.m;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < ncell * 2 * (kBandD + 1); t += kFX) {
      const int k = t / (2 * (kBandD + 1)), r = t % (2 * (kBandD + 1));
      const int mix = r / (kBandD + 1), n = r % (kBandD + 1);
      double mm = -INFINITY;
      for (int c = 0; c < nch; ++c) mm = fmax(mm, s_tmp[k * nch + c][mix][kBandD + 1]);
      double acc = 0.0;
      for (int c = 0; c < nch; ++c) {
        const double qm = s_tmp[k * nch + c][mix][kBandD + 1];
        acc += qm == -INFINITY ? 0.0 : s_tmp[k * nch + c][mix][n] * exp(qm - mm);
      }
      s_P[k][mix][n] = acc;
      if (n == 0) s_P[k][mix][kBandD + 1] = mm;
    }
    // the slow-component lists (one thread per cell and mixture); -1: a
    // chunk's list overflowed (that cell's survivors take the direct sum)
    for (int t = threadIdx.x; t < ncell * nch * 2; t += kFX) {
      const int u = t >> 1, mix = t & 1;
      s_ndu[u][mix] = W.cpart[u / nch][u % nch][mix].n_dir;
    }
    for (int t = threadIdx.x; t < ncell * nch * 2 * kChunkDir; t += kFX) {
      const int d = t % kChunkDir, r = t / kChunkDir, u = r >> 1, mix = r & 1;
      s_dir[u][mix][d] = W.cpart[u / nch][u % nch][mix].dir[d];
    }
    __syncthreads();
    // each list in component order (k_band lists them in atomic order): the
    // slow components are then summed in a fixed order, run to run
    for (int t = threadIdx.x; t < ncell * nch * 2; t += kFX) {
      const int u = t >> 1, mix = t & 1, nd = s_ndu[u][mix];
      int* L = s_dir[u][mix];
      for (int a = 1; a < nd; ++a) {
        const int v = L[a];
        int b = a - 1;
        while (b >= 0 && L[b] > v) {
          L[b + 1] = L[b];
          --b;
        }
        L[b + 1] = v;
      }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < ncell * 2; t += kFX) {
      const int k = t >> 1, mix = t & 1;
      int nd = 0;
      for (int c = 0; c < nch; ++c) {
        const int q = s_ndu[k * nch + c][mix];
        nd = (nd < 0 || q < 0) ? -1 : nd + q;
      }
      s_nd[k][mix] = nd;
    }
    for (int t = threadIdx.x; t < ncell; t += kFX) s_cells[t] = W.cells[t];
    __syncthreads();
    if (kb == 0) { TMARK(5) }
    const float g0 = (float)Tb.origin, h32 = (float)Tb.h;
    // this block's survivors, in rounds of kFStage staged in LDS by
    // coalesced loads all in flight at once
    const int per = (ns + kFinBlocks - 1) / kFinBlocks;
    const int i0 = min(ns, kb * per), i1 = min(ns, i0 + per);
    for (int r0 = i0; r0 < i1; r0 += kFStage) {
      const int rn = min(kFStage, i1 - r0);
      __syncthreads();  // (the previous round's reads of s_sy / s_si done)
      for (int t = threadIdx.x; t < rn; t += kFX) {
        s_sy[t] = W.sy[r0 + t];
        s_si[t] = W.sidx[r0 + t];
      }
      __syncthreads();
      for (int t = threadIdx.x; t < rn; t += kFX) {
        const float yf = s_sy[t];
        const int c = band_cell(Tb, yf);
        int lo = 0, hi = ncell;  // its listed position (k_band listed every survivor's cell)
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (s_cells[mid] < c) lo = mid + 1; else hi = mid;
        }
        const int k = lo;
        const double y = score_coord(yf, lgmm);
        const double u = (y - (double)cell_centre(g0, h32, c)) / Tb.h;
        auto horner = [&](int mix) {
          double p = s_P[k][mix][kBandD];
#pragma unroll
          for (int n = kBandD - 1; n >= 0; --n) p = fma(p, u, s_P[k][mix][n]);
          return p;
        };
        // log of the mixture from its expansion value p, plus its slow
        // components term by term; the direct sum when a chunk's list overflowed
        auto finish = [&](int mix, const tpe_seg& S, double p) -> double {
          const int ndt = s_nd[k][mix];
          if (ndt < 0) return band_direct(S, coef64, y);
          const double m = s_P[k][mix][kBandD + 1];
          // every component of the cell slow (a cell budget that forces wide
          // cells: in a tail cell the prior component itself): nothing was
          // expanded, so there is no scale m to sum the listed ones at
          if (m == -INFINITY) return band_direct(S, coef64, y);
          if (ndt > 0) {
            for (int cc = 0; cc < nch; ++cc) {
              const int un = k * nch + cc, nd = s_ndu[un][mix];
              for (int d = 0; d < nd; ++d) {
                const double4 cf = ld4(coef64, S.comp_off + s_dir[un][mix][d]);
                const double t = (y - cf.x) * cf.y;
                p += exp(cf.z - 0.5 * t * t - m);
              }
            }
          }
          return log(p) + m;
        };
        const double pb = horner(0), pa = horner(1);
        const double lb = finish(0, SB, pb);
        const double la = finish(1, SA, pa);
        best_update(bx, lb - la, s_si[t], cand_value(yf, lgmm));
      }
    }
  }
  if (kb == 0) { TMARK(6) }
  bx = block_best<kFX>(bx, red);
  if (threadIdx.x == 0) W.win[kb] = bx;
}

// The job's winner from its k_band_final blocks' (one wave per job).
__global__ __launch_bounds__(kWave) void k_band_pick(const tpe_job* __restrict__ jobs,
                                                     tpe_best* __restrict__ best,
                                                     BandWork* __restrict__ work) {
  const int j = blockIdx.x, lane = threadIdx.x;
  BandWork& W = work[j];
  if (W.over) return;
  BestT b{0.0, -1, 0.0};
  if (lane < kFinBlocks) b = W.win[lane];
  b = wave_best(b);
  if (lane == 0) {
    best[j] = tpe_best{b.score, b.index, b.value, jobs[j].n_cand};
#ifdef TPE_BAND_TIMING
    W.tmark[7] = wall_clock64();
#endif
  }
}

// The partial reduce every scorer ends with (launch_reduce), one block per
// job: combine its partials.  It lives here because k_band's fallbacks run
// the same thread_best<256> on the fp32 partials: with k_band its only caller
// in the translation unit the compiler seems to specialise thread_best's nper
// argument to k_band's (an int) before inlining: the unrolled loop's bound test
// compiles to other instructions (seen by removing the reduce from the old file).
__global__ __launch_bounds__(kBS) void k_reduce(const tpe_job* __restrict__ jobs,
                                                const tpe_best* __restrict__ partial, int64_t nper,
                                                tpe_best* __restrict__ best) {
  __shared__ BestT red[kBS / kWave];
  BestT b = thread_best<kBS>(partial + (int64_t)blockIdx.x * nper, nper);
  b = block_best<kBS>(b, red);
  if (threadIdx.x == 0) best[blockIdx.x] = tpe_best{b.score, b.index, b.value, jobs[blockIdx.x].n_cand};
}
}  // namespace

void launch_reduce(const tpe_job* jobs, const tpe_best* partial, int64_t nper, tpe_best* best,
                   int n_jobs, hipStream_t st) {
  hipLaunchKernelGGL(k_reduce, dim3(n_jobs), dim3(kBS), 0, st, jobs, partial, nper, best);
}
}  // namespace tpe

using namespace tpe;

extern "C" int64_t tpe_band_bytes(const tpe_job* host_jobs, int n_jobs, int64_t* ctl_bytes,
                                  int64_t* work_bytes) {
  if (n_jobs < 0 || (n_jobs > 0 && !host_jobs)) return -1;
  const int64_t tiles = n_jobs > 0 ? tpe_table_fast_tiles(host_jobs, n_jobs) * n_jobs : 1;
  if (ctl_bytes) *ctl_bytes = tiles * kHdrWords * (int64_t)sizeof(uint32_t);
  if (work_bytes) *work_bytes = (int64_t)sizeof(BandWork) * std::max(n_jobs, 1);
  return tiles * kTileSlots * (int64_t)sizeof(tpe_band);
}

// The band work's layout and the two stages' constants, for tests that read
// a job's route (BandWork.{ns, ncell, over, direct}) back: host only.
extern "C" int tpe_band_layout(int64_t* out, int n) {
  const int64_t v[] = {
      (int64_t)sizeof(BandWork),         (int64_t)offsetof(BandWork, ns),
      (int64_t)offsetof(BandWork, ncell), (int64_t)offsetof(BandWork, over),
      (int64_t)offsetof(BandWork, direct), (int64_t)offsetof(BandWork, sy),
      (int64_t)offsetof(BandWork, sidx),  (int64_t)offsetof(BandWork, cells),
      kBandBlocks, kBandDirect, kBandSurv, kBandCells, kBandSurvMax, kBandTiles, kChunkDir,
      kTileSlots, kTileF, kHdrWords, (int64_t)kTileFull};
  const int m = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < m && i < n; ++i)
    if (out) out[i] = v[i];
  return m;
}

extern "C" int tpe_band_rescore(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                                const tpe_seg* segs, const double* coef64,
                                const tpe_table* tables, const tpe_band* band,
                                const uint32_t* band_ctl, const tpe_best* partial,
                                int64_t n_partial, tpe_best* best, void* work, void* stream) {
  bool inj = false;
  if (!check_gmm_jobs("tpe_band_rescore", host_jobs, n_jobs, 65535, kJobTable, &inj))
    return TPE_E_ARG;
  if (n_jobs == 0) return TPE_OK;
  if (inj) {
    set_error("tpe_band_rescore: sampled jobs only");
    return TPE_E_ARG;
  }
  if (!jobs || !segs || !coef64 || !tables || !band || !band_ctl || !partial || !best || !work) {
    set_error("tpe_band_rescore: null pointer");
    return TPE_E_ARG;
  }
  const int64_t gx = tpe_table_fast_tiles(host_jobs, n_jobs);
  if (!check_partials("tpe_band_rescore", n_partial, gx * n_jobs)) return TPE_E_ARG;
  hipLaunchKernelGGL(k_band, dim3(kBandBlocks, n_jobs), dim3(kBX), 0, (hipStream_t)stream, jobs,
                     segs, coef64, tables, band, band_ctl, partial, (int)gx, best,
                     static_cast<BandWork*>(work));
  hipLaunchKernelGGL(k_band_final, dim3(kFinBlocks, n_jobs), dim3(kFX), 0, (hipStream_t)stream,
                     jobs, segs, coef64, tables, static_cast<BandWork*>(work));
  hipLaunchKernelGGL(k_band_pick, dim3(n_jobs), dim3(kWave), 0, (hipStream_t)stream, jobs, best,
                     static_cast<BandWork*>(work));
  return check_launch("tpe_band_rescore");
}
