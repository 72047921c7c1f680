// tpe_table.hip -- the cell table's plan, build and score cells.
//
// Turns each job's two mixtures (GMM1_lpdf / LGMM1_lpdf's component sums,
// hyperopt/tpe.py:117-180, 265-307) into the per-cell polynomials and cubics
// the table scorers read (the method and the layout: tpe_table.hpp).
//
// Exports: tpe_table_scratch_bytes, tpe_table_build; launch_table_plan for
// the pruned fp64 scorer.
#include "tpe_table.hpp"

namespace tpe {
namespace {
constexpr double kRhoLim = 5.8;      // admissible 9|A| + 65|B|
#ifndef TPE_TAU_TABLE
#define TPE_TAU_TABLE 17.0
#endif
constexpr double kTauExtra = TPE_TAU_TABLE;  // exclusion margin (nats) on top of log(M)
constexpr double kDrawZ = 5.8;       // |z| of an fp32 Box-Muller draw is < 5.77
#ifndef TPE_BUILD_BLOCKS
#define TPE_BUILD_BLOCKS 384
#endif
// build blocks per job (grid-stride over cells).  384, not 512: a C3 uniform
// label has ~180 quads (one per block) and a normal label ~625 block rounds,
// so 512 launched ~330 idle blocks per uniform job and left the normal jobs'
// second round uneven; table-build group 0.229 -> 0.214 ms per C3 level,
// C5 unchanged (1.74 -> 1.68-1.73 ms), two-round A/B on one box (late round 5)
constexpr int kBuildBlocks = TPE_BUILD_BLOCKS;
constexpr int kCoopCells = 4096;     // labels with at most this many cells build a quad per block

// s = h*inv such that 9 s (z + s) + 32.5 s^2 <= kRhoLim (|y0-mu| inv <= z + s)
__device__ __forceinline__ double admissible_s(double z) {
  return (-9.0 * z + sqrt(81.0 * z * z + 166.0 * kRhoLim)) / 83.0;
}

// ---------------------------------------------------------------------------
// plan: coordinate range, admissible half-width, reach windows, wide list.
// Two launches over (component tiles, 2 * n_jobs) -- y = 2*job + half, half 0
// the below mixture, 1 the above: P1 does every component's reach / bound and
// the tile-local scans, P2 applies the other tiles' carries.
// ---------------------------------------------------------------------------
constexpr int kPlanStride = 4;  // per tile: {max reach_hi, min reach_lo, #wide, min h}

// range of the scoring coordinate (where the below sampler can put a
// candidate: mu +- 5.8 sigma per component, clipped to the bounds) and the
// global lower bound T of a term that can matter (the prior's smallest term
// over the range, minus log(M) + kTauExtra); identical in every block
// draw_z: |z| bound of the sampler's normals (kDrawZ for fp32 draws, kDrawZ64
// for fp64 ones); tau: the exclusion margin (kTauExtra for the table,
// kTauExact for the pruned exact fp64 scorer)
__device__ __forceinline__ void plan_range(const tpe_job& J, const tpe_seg& SB, const tpe_seg& S,
                                           const double* __restrict__ mu,
                                           const double* __restrict__ sigma,
                                           const double* __restrict__ coef64, double* red,
                                           double draw_z, double tau, double& a, double& b,
                                           double& T) {
  a = INFINITY;
  b = -INFINITY;
  for (int k = threadIdx.x; k < SB.n_obs + 1; k += kBS) {
    const double m = mu[SB.comp_off + k], sg = sigma[SB.comp_off + k];
    a = fmin(a, m - draw_z * sg);
    b = fmax(b, m + draw_z * sg);
  }
  a = -block_max<kBS, double>(-a, red);
  b = block_max<kBS, double>(b, red);
  if (J.flags & TPE_F_INJECTED) {
    a = fmax(a, J.bin_lo);
    b = fmin(b, J.bin_hi);
  }
  if (J.flags & TPE_F_LOW) a = fmax(a, J.low);
  if (J.flags & TPE_F_HIGH) b = fmin(b, J.high);
  if (!(isfinite(a) && isfinite(b) && b >= a)) {
    // empty or degenerate: one cell at a finite point, candidates off it are exact
    const double c = isfinite(a) ? a : (isfinite(b) ? b : SB.prior_mu);
    a = b = c;
  }
  const double4 cp = ld4(coef64, S.comp_off + S.prior_pos);
  const double far = fmax(fabs(a - cp.x), fabs(b - cp.x)) * cp.y;
  T = cp.z - 0.5 * far * far - (log((double)(S.n_obs + 1)) + tau);
}

// component k of mixture S: wide flag, reach interval, admissible half-width
__device__ __forceinline__ void plan_comp(const tpe_seg& S, const double* __restrict__ sigma,
                                          const double* __restrict__ coef64, double T, int k,
                                          bool& wide, double& hr, double& lr, double& hk) {
  const double4 c = ld4(coef64, S.comp_off + k);
  const double d = c.z - T;
  const double z = d > 0.0 ? sqrt(2.0 * d) : 0.0;
  hk = d > 0.0 ? admissible_s(z) / c.y : INFINITY;
  wide = is_wide(S, k, c.y);
  const double r = z / c.y * (1.0 + 1e-9) + 1e-12 * fabs(c.x);
  hr = wide ? -INFINITY : c.x + r;
  lr = wide ? INFINITY : c.x - r;
}

__global__ __launch_bounds__(kBS) void k_table_plan1(
    const tpe_job* __restrict__ jobs, const tpe_seg* __restrict__ segs,
    const double* __restrict__ mu, const double* __restrict__ sigma,
    const double* __restrict__ coef64, double* __restrict__ reach_hi,
    double* __restrict__ reach_lo, double* __restrict__ part, tpe_table* __restrict__ tables,
    double draw_z, double tau) {
  __shared__ double red[kBS / kWave];
  __shared__ double scan_d[kBS / kWave];
  const int job = blockIdx.y >> 1, half = blockIdx.y & 1;
  const tpe_job J = jobs[job];
  const tpe_seg SB = segs[J.below];
  const tpe_seg S = segs[half ? J.above : J.below];
  const int nc = S.n_obs + 1;
  if ((int)blockIdx.x * kBS >= nc) return;  // block-uniform
  double a, b, T;
  plan_range(J, SB, S, mu, sigma, coef64, red, draw_z, tau, a, b, T);
  const int k = blockIdx.x * kBS + threadIdx.x;
  bool wide = true;
  double hr = -INFINITY, lr = INFINITY, hk = INFINITY;
  if (k < nc) plan_comp(S, sigma, coef64, T, k, wide, hr, lr, hk);
  hr = block_prefix_max(hr, scan_d);  // tile-local prefix max
  if (k < nc) reach_hi[S.comp_off + k] = hr;
  // tile-local suffix min: thread t handles element tile_end - t
  const int tend = min(nc, (int)(blockIdx.x + 1) * kBS) - 1;
  const int kr = tend - (int)threadIdx.x;
  bool wr;
  double hr2, lr2 = INFINITY, hk2;
  if (kr >= (int)blockIdx.x * kBS) plan_comp(S, sigma, coef64, T, kr, wr, hr2, lr2, hk2);
  lr2 = -block_prefix_max(-lr2, scan_d);
  if (kr >= (int)blockIdx.x * kBS) reach_lo[S.comp_off + kr] = lr2;
  const double tmax = block_max<kBS, double>(hr, red);
  const double tmin = -block_max<kBS, double>(-lr2, red);
  const double nw = block_sum<kBS, double>((k < nc && wide) ? 1.0 : 0.0, red);
  const double hmin = -block_max<kBS, double>(-hk, red);
  if (threadIdx.x == 0) {
    double* P = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kPlanStride;
    P[0] = tmax;
    P[1] = tmin;
    P[2] = nw;
    P[3] = hmin;
    if (blockIdx.x == 0) {
      if (half == 0) {
        tables[job].lo = a;
        tables[job].hi = b;
        tables[job].T_below = T;
      } else {
        tables[job].T_above = T;
      }
    }
  }
}

__global__ __launch_bounds__(kBS) void k_table_plan2(
    const tpe_job* __restrict__ jobs, const tpe_seg* __restrict__ segs,
    const double* __restrict__ mu, const double* __restrict__ sigma,
    const double* __restrict__ coef64, double* __restrict__ reach_hi,
    double* __restrict__ reach_lo, int32_t* __restrict__ wide_idx,
    const double* __restrict__ part, tpe_table* __restrict__ tables) {
  __shared__ double red[kBS / kWave];
  __shared__ int scan_n[kBS / kWave];
  const int job = blockIdx.y >> 1, half = blockIdx.y & 1;
  const tpe_job J = jobs[job];
  const tpe_seg S = segs[half ? J.above : J.below];
  const int nc = S.n_obs + 1;
  const int tiles = (nc + kBS - 1) / kBS;
  const int t = blockIdx.x;
  if (t >= tiles) return;  // block-uniform
  const double* P = part + (int64_t)blockIdx.y * gridDim.x * kPlanStride;
  double chi = -INFINITY, clo = INFINITY, woff = 0.0, hmin = INFINITY, nw = 0.0;
  for (int q = threadIdx.x; q < tiles; q += kBS) {
    if (q < t) {
      chi = fmax(chi, P[q * kPlanStride]);
      woff += P[q * kPlanStride + 2];
    }
    if (q > t) clo = fmin(clo, P[q * kPlanStride + 1]);
    hmin = fmin(hmin, P[q * kPlanStride + 3]);
    nw += P[q * kPlanStride + 2];
  }
  chi = block_max<kBS, double>(chi, red);
  clo = -block_max<kBS, double>(-clo, red);
  const int wbase = (int)block_sum<kBS, double>(woff, red);
  hmin = -block_max<kBS, double>(-hmin, red);
  const int ntot = (int)block_sum<kBS, double>(nw, red);
  const int k = t * kBS + threadIdx.x;
  bool wide = false;
  if (k < nc) {
    reach_hi[S.comp_off + k] = fmax(reach_hi[S.comp_off + k], chi);
    reach_lo[S.comp_off + k] = fmin(reach_lo[S.comp_off + k], clo);
    wide = is_wide(S, k, ld4(coef64, S.comp_off + k).y);
  }
  const int incl = block_prefix_sum(wide ? 1 : 0, scan_n);
  if (wide) wide_idx[S.comp_off + wbase + incl - 1] = k;
  if (t == 0 && threadIdx.x == 0) {
    if (half == 0) {
      tables[job].h_below = hmin;
      tables[job].n_wide_below = ntot;
      // raised by k_table_build (build_items, build_ab) and k_table_score
      // (eps_cubic) with atomics: zeroed here, one launch before
      tables[job].build_items = 0;
      tables[job].build_ab = 0.0f;
      tables[job].eps_cubic = 0.0f;
    } else {
      tables[job].h_above = hmin;
      tables[job].n_wide_above = ntot;
    }
  }
}

// The nine P_n sums of a wave at once (transposed butterfly).  Per DPP stage
// each lane keeps half of its live values and adds its partner's copy of
// them: stage 1 pairs lane i with 15-i of its row (row mirror, bit 3 chooses
// the half), stage 2 with 7-i of its half-row (half mirror, bit 2), stages 3
// and 4 with i^2 and i^1 (quad perms); a stage's partner always holds the same
// subset as the lane, because the mirrors come first.  After four stages lane
// p of each row holds its row's sum of P_rev4(p) (rev4: the 4-bit reversal);
// (row_sum9_transposed: the build sums each row on its own, one cell per
// row): 9 exchange-adds instead of the 9 x 4 of one DPP sum per term.
template <int CTRL, int M>
__device__ __forceinline__ void fold_stage(double (&w)[16], bool hi) {
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const double keep = hi ? w[2 * j + 1] : w[2 * j], send = hi ? w[2 * j] : w[2 * j + 1];
    w[j] = keep + dpp_d<CTRL>(send);
  }
}
__device__ __forceinline__ int rev4(int p) {
  return ((p & 1) << 3) | ((p & 2) << 1) | ((p & 4) >> 1) | ((p & 8) >> 3);
}

// The two reach windows of the span [ylo, yhi] (a run of cells) at once: four
// searches of wave_first's kind in one pass, one per 16-lane group -- g = 0 /
// 2: the first k of the below / above mixture with reach_hi[k] >= ylo, g = 1 /
// 3: the first k with reach_lo[k] > yhi (the window ends one before it).  16-ary narrowing:
// 10^4 components take 4 dependent probes, for all four searches together
// instead of 3 for each.  Every lane gets all four answers.
struct Windows {
  int lo_b, end_b, lo_a, end_a;
};
__device__ __forceinline__ Windows cell_windows(const tpe_seg& SB, const tpe_seg& SA,
                                                const double* __restrict__ reach_hi,
                                                const double* __restrict__ reach_lo, double ylo,
                                                double yhi) {
  const int lane = lane_id(), g = lane >> 4, l = lane & 15;
  const tpe_seg& S = g < 2 ? SB : SA;
  const bool gt = g & 1;
  const double* a = (gt ? reach_lo : reach_hi) + S.comp_off;
  const double v = gt ? yhi : ylo;
  int lo = 0, hi = S.n_obs + 1;  // answer in [lo, hi]
  while (__any(lo < hi)) {
    const bool active = lo < hi;
    const int stride = (hi - lo + 15) / 16;
    const int idx = lo + l * stride;
    bool p = true;  // probes past the end qualify
    if (active && idx < hi) p = gt ? (a[idx] > v) : (a[idx] >= v);
    const uint32_t m = (uint32_t)(__ballot(p) >> (g * 16)) & 0xFFFFu;
    const int f = m ? __builtin_ctz(m) : 16;
    if (active) {
      if (f == 0) {
        hi = lo;  // a[lo] qualifies
      } else {
        const int nlo = lo + (f - 1) * stride + 1;
        hi = min(lo + f * stride, hi);
        lo = nlo;
      }
    }
  }
  return Windows{__builtin_amdgcn_readlane(lo, 0), __builtin_amdgcn_readlane(lo, 16),
                 __builtin_amdgcn_readlane(lo, 32), __builtin_amdgcn_readlane(lo, 48)};
}

// Row-level reduction (each 16-lane DPP row on its own): the nine P_n sums
// of the row, lane p holding the sum of P_rev4(p) (wave_sum9_transposed
// without the cross-row steps).
__device__ __forceinline__ double row_sum9_transposed(const double (&P)[9]) {
  const int lane = lane_id();
  double w[16];
#pragma unroll
  for (int n = 0; n < 16; ++n) w[n] = n < 9 ? P[n] : 0.0;
  fold_stage<kDppMirror, 5>(w, (lane >> 3) & 1);      // 9 live -> 5
  w[5] = 0.0;
  fold_stage<kDppHalfMirror, 3>(w, (lane >> 2) & 1);  // -> 3
  w[3] = 0.0;
  fold_stage<kDppXor2, 2>(w, (lane >> 1) & 1);        // -> 2
  fold_stage<kDppXor1, 1>(w, lane & 1);               // -> 1
  return w[0];
}

// One wave builds one mixture's expansion on four consecutive cells, one per
// 16-lane row (y0: the row's cell centre); returns the row's failed flag.
// k_lo .. k_hi: the reach window of the four cells' span (cell_windows) --
// a superset of each cell's own, whose components the exclusion test below
// drops -- then the wide list; every row walks the same items.
struct BuildLds {  // the block's four waves' partial expansions of one mixture
  int m[kBS / kWave][4];         // per wave and row: its scale (a power of two's exponent)
  double p[kBS / kWave][kWave];  // per wave and lane: its row's sum of P_rev4(lane & 15)
  int bad[kBS / kWave][4];
};
constexpr int kNoScale = -100000;  // a lane that has summed nothing yet
__device__ __forceinline__ bool build_mix(const tpe_seg& S, const double* __restrict__ coef64,
                                          int k_lo, int k_hi,
                                          const int32_t* __restrict__ wide_idx, int n_wide,
                                          double T, double y0, double h, float* cell, bool store,
                                          int mix, double& m_out, BuildLds& X, bool coop,
                                          int& itm) {
  // coop (block-uniform): the block's four waves build the same four cells
  // and split the items; otherwise every wave builds its own four cells
  constexpr int kNW = kBS / kWave;
  // (the wave's index read as a scalar: what depends on it alone stays out of
  // the vector registers)
  const int wv = coop ? __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave) : 0;
  const int stride = coop ? 16 * kNW : 16;
  const int64_t off = S.comp_off;
  const int nwin = max(0, k_hi - k_lo + 1);
  const int items = nwin + n_wide;
  itm = max(itm, items);  // (the error bound's summation depth, mix_eps)
  const int lane = lane_id(), l = lane & 15, row = lane >> 4;
  // component of work item `it` (window first, then the wide list)
  auto comp = [&](int it) -> int {
    return it < nwin ? k_lo + it : wide_idx[off + (it - nwin)];
  };
  const float hf = (float)h, Tf = (float)T;
  // One pass over the items.  Each lane keeps its own scale 2^sl (sl an
  // integer, raised when a term would exceed 2^8 of it) and rescales its
  // partial sums by exact powers of two; the row's lanes (and the block's
  // waves, coop) meet at the largest scale the same way, and the cell's sums
  // are finally normalised by the power of two that puts P_0 in [1, 2) --
  // every rescaling exact, P_0 >= 1 as the storage bound assumes.  The
  // exponent is formed in fp64, the series and the per-component tests in
  // fp32.  P_0..P_3 are summed in fp64 (a sum of ~10^2 fp32 terms per lane
  // would carry ~10^2 roundings into mix_eps), P_4..P_8 in fp32: at most 2 %
  // of the terms' absolute sum lies there (tools/table_bounds.py), so their
  // rounding costs mix_eps K 2^-24 0.0198.  The next item's coefficients are
  // loaded before this item's work.
  constexpr int kP64 = 4;
  double P[kP64];
  float Q[kP - kP64];
#pragma unroll
  for (int n = 0; n < kP64; ++n) P[n] = 0.0;
#pragma unroll
  for (int n = 0; n < kP - kP64; ++n) Q[n] = 0.0f;
  auto acc = [&](int n, float t) __attribute__((always_inline)) {
    if (n < kP64)
      P[n] += (double)t;
    else
      Q[n - kP64] += t;
  };
  auto rescale = [&](int d) __attribute__((always_inline)) {  // multiply the sums by 2^d
#pragma unroll
    for (int n = 0; n < kP64; ++n) P[n] = ldexp(P[n], d);
#pragma unroll
    for (int n = 0; n < kP - kP64; ++n) Q[n] = ldexpf(Q[n], d);
  };
  int sl = kNoScale;
  bool bad = false;
  int it = wv * 16 + l;  // the block's four waves split the items, 16 lanes per cell each
  int k = it < items ? comp(it) : 0;
  double4 c = it < items ? ld4(coef64, off + k) : make_double4(0.0, 0.0, 0.0, 0.0);
  for (; it < items; it += stride) {
    const int itn = it + stride;
    const int kn = itn < items ? comp(itn) : 0;
    const double4 cn = itn < items ? ld4(coef64, off + kn) : c;
    // window items that are wide come from the list instead; an item below
    // the plan's floor on the whole cell is left out (branch-free: an
    // excluded item adds zero terms)
    const bool skip = it < nwin && is_wide(S, k, c.y);
    const double dy = y0 - c.x;
    const float dyf = (float)dy, inv = (float)c.y;
    const float zn = fmaxf(fabsf(dyf) - hf, 0.0f) * inv;
    const bool inc = !skip && ((float)c.z - 0.5f * zn * zn >= Tf);
    const double zc = dy * c.y;
    const double t2 = (c.z - 0.5 * zc * zc) * kLog2e;  // log2 of the term at the centre
    const bool up = inc && t2 > (double)(sl + 8);
    if (__any(up)) {
      if (up) {
        const int ns = (int)ceil(t2);
        rescale(max(sl - ns, -1100));
        sl = ns;
      }
    }
    const float hi2 = hf * inv * inv;
    const float Af = inc ? -dyf * hi2 : 0.0f, B2 = inc ? -hf * hi2 : 0.0f;  // A and 2B
    bad = bad || (9.0f * fabsf(Af) + 32.5f * fabsf(B2) > (float)(kRhoLim * (1.0 + 1e-5)));
    // the term 2^(t2 - sl) = 2^n 2^f, n = floor(t2 - sl) exact and f in [0, 1)
    // rounded once to fp32: a relative error <= ln2 2^-24 (+ v_exp_f32's),
    // whatever the term's size
    const double xs = t2 - (double)sl, xn = floor(xs);
    const float e = inc ? ldexpf(__builtin_amdgcn_exp2f((float)(xs - xn)), (int)xn) : 0.0f;
    float cm = 0.0f, cc = e;  // e * c_n
    acc(0, e);
#pragma unroll
    for (int n = 0; n + 1 < kP; ++n) {
      const float cnx = fmaf(Af, cc, B2 * cm) * (1.0f / (float)(n + 1));
      acc(n + 1, cnx);
      cm = cc;
      cc = cnx;
    }
    k = kn;
    c = cn;
  }
  // the row's lanes at the row's largest scale (exact); then the block's
  // waves at theirs (coop)
  int sr = row_max_i(sl);
  rescale(max(sl - sr, -1100));
  static_assert(kP == 9, "row_sum9_transposed folds nine terms");
  double Pall[kP];
#pragma unroll
  for (int n = 0; n < kP; ++n) Pall[n] = n < kP64 ? P[n] : (double)Q[n - kP64];
  double tot = row_sum9_transposed(Pall);  // lane p of the row: the row's total of P_rev4(p)
  bad = ((__ballot(bad) >> (lane & ~15)) & 0xFFFFull) != 0;
  bool anybad = bad;
  if (coop) {
    if (l == 0) {
      X.bad[wv][row] = bad;
      X.m[wv][row] = sr;
    }
    X.p[wv][lane] = tot;
    __syncthreads();
    int sb = X.m[0][row];
#pragma unroll
    for (int w = 1; w < kNW; ++w) sb = max(sb, X.m[w][row]);
    tot = 0.0;
    anybad = false;
    for (int w = 0; w < kNW; ++w) {
      tot += ldexp(X.p[w][lane], max(X.m[w][row] - sb, -1100));
      anybad = anybad || X.bad[w][row];
    }
    sr = sb;
    __syncthreads();  // (X is reused by the next call)
  }
  // normalise: P_0 (the row's lane 0) in [1, 2)
  const double p0 = __shfl(tot, lane & ~15, kWave);
  int e0 = 0;
  if (p0 > 0.0) {
    (void)frexp(p0, &e0);  // p0 = f 2^e0, f in [0.5, 1)
    e0 -= 1;
    tot = ldexp(tot, -e0);
  }
  const int n = rev4(l);
  if (store && wv == 0 && n < kP) {
    if (n < kP32)
      cell[2 * n + mix] = (float)tot;
    else
      reinterpret_cast<_Float16*>(cell + 2 * kP32)[2 * (n - kP32) + mix] = (_Float16)(float)tot;
  }
  m_out = (p0 > 0.0) ? (double)(sr + e0) * kLn2 : -INFINITY;
  return anybad;
}

// ---------------------------------------------------------------------------
// score cells.  The argmax needs only the score
//     f(u) = (m_b - m_a) + log P_b(u) - log P_a(u)
// per candidate, and on a cell f is far smoother than either mixture (a
// difference of two log-densities, sampled at half-widths of ~0.06 of the
// narrowest bandwidth): a cubic interpolant at four Chebyshev nodes of
// [-1.05, 1.05] reproduces it to ~1e-7 on C3's histories.
// k_table_score gives each cell kScoreLanes = 8 lanes: lanes 0-3 evaluate f
// at the nodes from the cell's STORED coefficients (fp32 Horner, the log of
// the ratio as exponent + v_log_f32 of the mantissa); the nodes' values are
// broadcast, every lane forms the same cubic (fp64 divided differences) and
// rounds it to fp32.  Then the cubic's error is BOUNDED, not sampled: lane i
// takes the sub-interval of [-1.0501, 1.0501] centred at c_i (half-width
// r = 1.0501 / 8) and encloses
//     e(c_i + t) = f^(c_i + t) - q(c_i + t),   |t| <= r,
// f^ = off + ln P^_b - ln P^_a being the score of the stored polynomials
// (exact reals).  Per mixture: the Taylor coefficients T_k of P^ at c_i (a
// Horner shift), a_k = T_k / T_0, the log series ln P^(c+t) = ln T_0 +
// sum_k l_k t^k with l_k = a_k - (1/k) sum_{j<k} j l_j a_{k-j} (exact up to
// fp64 rounding) for k <= kLogD, and the rest bounded by the majorant
// -ln(1 - w~(t)), w~ = sum |a_k| t^k: its coefficients m_k >= |l_k| (same
// recurrence on |a_k|, all terms positive), summed for kLogD < k <= kLogM,
// and past kLogM by Cauchy's estimate on the radius 4r (m_k (4r)^k <=
// -ln(1 - w~(4r)) <= ln 2 when w~(4r) <= 1/2; otherwise the cell is flagged).
// So |e| <= |E_0| + sum_{k<=kLogD} |E_k| r^k + rem_b + rem_a + rounding, E_k
// the coefficients of the difference polynomial; the cell's bound is the
// largest of its lanes'.  A cell whose bound exceeds kFitTol (or whose P is
// not positive, or whose cubic is not finite) is flagged (NaN c0) and its
// candidates take the two-polynomial cell.  The job's tpe_table gets
//   slope     = max |c1| + 2.11 |c2| + 3.31 |c3|  (>= |q'(u)| on |u| <= 1.0501)
//   eps_cubic = max over unflagged cells of  fit + 2^-21 sum_k |c_k| 1.0501^k
//               + 4.5 2^-24 slope_cell + 2^-24 |off| (1 + 1e-4)
// (the cubic's fp32 Horner beyond its 2^-22 |s| part, u's fp32 rounding, the
// fp32 score offset) and eps_mix, the per-mixture polynomial bound
// (mix_eps).  16 B per cell, after the job's cells and m pairs in its
// 128-B-per-cell region.
// ---------------------------------------------------------------------------
constexpr double kFitTol = 1.0e-6;   // cubic-vs-polynomial bound allowed (nats)
constexpr int kScoreLanes = 8;       // lanes per cell: 4 nodes, 8 sub-intervals
constexpr int kScoreCellsPerBlock = kBS / kScoreLanes;
#ifndef TPE_SCORE_BLOCKS
#define TPE_SCORE_BLOCKS 160
#endif
// per job (grid-stride over cells).  160, not 256: a C3 normal label's ~10 000
// cells are ~313 block rounds (two even rounds instead of 1.2), a uniform
// label's 710 cells need 23 blocks; build group -5 us per C3 level, C5
// unchanged (three one-box A/Bs, late round 5)
constexpr int kScoreBlocks = TPE_SCORE_BLOCKS;
constexpr double kUFit = 1.0501;     // |u| the bounds cover (u's fp32 rounding: <= 1.05 (1 + 5 2^-24))
constexpr int kLogD = 7;             // log-series terms carried exactly
constexpr int kLogM = 12;            // majorant terms summed (then Cauchy's tail)
constexpr double kU32 = 0x1.0p-24;   // fp32 unit roundoff
// max of a + b = 1.0501|A| + 1.1028|B| over the admissible set 9|A| + 65|B| <=
// 5.8 (1 + 2e-5) (the build's test with its fp32 slack): at |A| = 0.64446
constexpr double kAbMax = 0.6768;

// Per-mixture relative error bound of a stored cell polynomial against its
// mixture, |P^(u) - S(y) e^-m| <= eps_mix S(y) e^-m on |u| <= kUFit, from the
// build's worst case over the job's cells (DESIGN.md 3.1 derives each term):
// items = most components one cell summed, coop = the cooperative build (64
// lanes per row), ab = max 1.0501|A| + 1.1028|B| of a summed component (also
// >= a + 2b).  Terms relative to a component's value carry e^ab (its
// majorant over its value at u); those of the P_n sums carry E2 = e^2ab.
__host__ __device__ inline double mix_eps(int items, bool coop, double ab) {
  const double u = kU32, ud = 0x1.0p-53;
  const int stride = coop ? 64 : 16;
  const int K = (items + stride - 1) / stride + 5 + (coop ? 5 : 0);  // fp64 adds into one P_n
  const double E1 = exp(ab), E2 = E1 * E1;
  return 4.4e-7                         // series truncation (tools/table_bounds.py)
         + exp(-kTauExtra) * 1.0001     // components below the exclusion floor: at most M, each
                                        // < e^-tau / M of S (4.2e-8 at tau = 17)
         + 0.6932 * u + 1e-13           // each term's exponent: its fraction rounded to fp32
         + 0x1.0p-22                    // v_exp_f32 (checked exhaustively, tpe_check_transcendentals)
         + 5.5 * u * ab                 // A, B rounded to fp32
         + 4.0 * u * ab * E2            // the fp32 series recurrence (4 roundings per step)
         + u * E2                       // P_0..P_5 stored in fp32
         + (K + 1) * u * 0.0198 * 1.0001  // P_4..P_8 summed in fp32 (tools/table_bounds.py)
         + 1.5e-7 + 0x1.0p-25 * 4.2 * E1  // P_6..P_8 in fp16 (+ subnormal spacing)
         + (K + 8) * 2.0 * ud * E2;     // fp64 sums, rescale and merge factors of the P_n
}

// one mixture's stored coefficients as doubles (exact)
__device__ __forceinline__ void cell_coefs(const float* cell, int mix, double (&p)[kP]) {
  const _Float16* tail = reinterpret_cast<const _Float16*>(cell + 2 * kP32);
#pragma unroll
  for (int n = 0; n < kP32; ++n) p[n] = (double)cell[2 * n + mix];
#pragma unroll
  for (int n = kP32; n < kP; ++n) p[n] = (double)(float)tail[2 * (n - kP32) + mix];
}

// ln P^(c + t) = lnT0 + sum_{k=1..kLogD} l[k] t^k + R, |R| <= rem on |t| <= r;
// false when P^(c) <= 0 or the majorant's radius check fails
__device__ __forceinline__ bool log_taylor(const double (&p)[kP], double c, double r, double& lnT0,
                                           double (&l)[kLogD + 1], double& rem) {
  double T[kP];
#pragma unroll
  for (int n = 0; n < kP; ++n) T[n] = p[n];
#pragma unroll
  for (int i = 0; i < kP - 1; ++i)
#pragma unroll
    for (int j = kP - 2; j >= i; --j) T[j] = fma(c, T[j + 1], T[j]);
  if (!(T[0] > 0.0) || !isfinite(T[0])) return false;
  lnT0 = log(T[0]);
  const double inv0 = 1.0 / T[0];
  double a[kP];
  a[0] = 1.0;
#pragma unroll
  for (int k = 1; k < kP; ++k) a[k] = T[k] * inv0;
  l[0] = 0.0;
#pragma unroll
  for (int k = 1; k <= kLogD; ++k) {
    double s = 0.0;
#pragma unroll
    for (int j = 1; j < k; ++j) s = fma((double)j * l[j], a[k - j], s);
    l[k] = a[k] - s * (1.0 / (double)k);
  }
  // majorant of the log series (fp32: a bound, inflated by 1e-3 below)
  float aa[kP], m[kLogM + 1];
  float w4 = 0.0f, rr = 1.0f;
  const float r4 = (float)(4.0 * r);
#pragma unroll
  for (int k = 1; k < kP; ++k) {
    aa[k] = (float)fabs(a[k]);
    rr *= r4;
    w4 = fmaf(aa[k], rr, w4);
  }
  w4 *= 1.001f;
  if (!(w4 <= 0.5f)) return false;
  float tail = 0.0f, rk = 1.0f, jm[kLogM + 1];  // jm[j] = j m_j
  const float rf = (float)r;
#pragma unroll
  for (int k = 1; k <= kLogM; ++k) {
    // m_k = |a_k| + (1/k) sum_j j m_j |a_{k-j}| (fp32 rounding inside the
    // 1e-3 inflation below)
    float s = 0.0f;
#pragma unroll
    for (int j = 1; j < k; ++j)
      if (k - j < kP) s = fmaf(jm[j], aa[k - j], s);
    const float mk = fmaf(s, 1.0f / (float)k, k < kP ? aa[k] : 0.0f);
    m[k] = mk;
    jm[k] = (float)k * mk;
    rk *= rf;
    if (k > kLogD) tail = fmaf(mk, rk, tail);
  }
  // past kLogM: m_k (4r)^k <= ln 2, so sum_{k > kLogM} m_k r^k <= ln2 4^-(M+1) / (3/4)
  rem = (double)tail * 1.001 + 0.6931471805599453 * ldexp(1.0, -2 * (kLogM + 1)) / 0.75;
  return true;
}

#ifndef TPE_TSCORE_WPE  // diagnostic builds: waves-per-EU target of the cubics kernel
#define TPE_TSCORE_WPE 4
#endif
__global__ __launch_bounds__(kBS) __attribute__((amdgpu_waves_per_eu(TPE_TSCORE_WPE))) void k_table_score(const tpe_job* __restrict__ jobs,
                                                     tpe_table* __restrict__ tables,
                                                     float* __restrict__ cells,
                                                     unsigned long long* __restrict__ stats) {
  __shared__ float fred[kBS / kWave];
  const tpe_job J = jobs[blockIdx.y];
  const tpe_table Tb = tables[blockIdx.y];
  const int nb = Tb.nb;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // the per-mixture bound from the build's worst case (k_table_build's atomics)
    tables[blockIdx.y].build_ab = (float)kAbMax;
    tables[blockIdx.y].eps_mix =
        (float)(mix_eps(Tb.build_items, nb <= kCoopCells, kAbMax) * (1.0 + 1e-6));
  }
  char* region = reinterpret_cast<char*>(cells) + J.tbl_off * kSlotB;
  float4* outs = const_cast<float4*>(score_cells_of(region, J.tbl_cap));
  const int sub = threadIdx.x / kScoreLanes, l = threadIdx.x % kScoreLanes;
  const int gbase = lane_id() & ~(kScoreLanes - 1);  // first lane of this cell's group
  constexpr double kU = (double)kULim;
  const double nd0 = kU * 0.92387953251128674, nd1 = kU * 0.38268343236508978, nd2 = -nd1,
               nd3 = -nd0;
  const double un = l == 0 ? nd0 : l == 1 ? nd1 : l == 2 ? nd2 : nd3;  // (lanes >= 4: unused)
  const double i10 = 1.0 / (nd1 - nd0), i21 = 1.0 / (nd2 - nd1), i32 = 1.0 / (nd3 - nd2),
               i20 = 1.0 / (nd2 - nd0), i31 = 1.0 / (nd3 - nd1), i30 = 1.0 / (nd3 - nd0);
  const float uf = (float)un;
  // LGMM1: the exact score is taken at log(exp(y)) of the returned value, not
  // at y (cand_value) -- a shift of u by at most du_lg (lgmm_du)
  const float du_lg = lgmm_du(J, Tb);
  constexpr double r = kUFit / kScoreLanes;
  const double cI = -kUFit + (2 * l + 1) * r;  // this lane's sub-interval centre
  float slope = 0.0f, epsc = 0.0f;  // over this thread's unflagged cells (lane 0 of a group)
  // group-uniform trip count: every lane of a group runs the shuffles
  for (int64_t c = (int64_t)blockIdx.x * kScoreCellsPerBlock + sub; c < nb;
       c += (int64_t)gridDim.x * kScoreCellsPerBlock) {
    const float* cell = reinterpret_cast<const float*>(region) + c * kCellF;
    const double off = (double)cell[15];
    const _Float16* tail = reinterpret_cast<const _Float16*>(cell + 2 * kP32);
    float pb = 0.0f, pa = 0.0f;
#pragma unroll
    for (int n = kP - 1; n >= kP32; --n) {
      pb = fmaf(pb, uf, (float)tail[2 * (n - kP32)]);
      pa = fmaf(pa, uf, (float)tail[2 * (n - kP32) + 1]);
    }
#pragma unroll
    for (int n = kP32 - 1; n >= 0; --n) {
      pb = fmaf(pb, uf, cell[2 * n]);
      pa = fmaf(pa, uf, cell[2 * n + 1]);
    }
    const bool ok_pt = (pb > 0.0f) && (pa > 0.0f) && isfinite(pb) && isfinite(pa);
    // log(pb / pa) = ln2 * (e + log2(m)), m = the ratio's mantissa in [0.5, 1)
    int e = 0;
    const float mt = ok_pt ? frexpf(pb / pa, &e) : 1.0f;
    const double f = off + kLn2 * ((double)e + (double)__builtin_amdgcn_logf(mt));
    const double f0 = __shfl(f, gbase + 0, kWave), f1 = __shfl(f, gbase + 1, kWave),
                 f2 = __shfl(f, gbase + 2, kWave), f3 = __shfl(f, gbase + 3, kWave);
    const bool nodes_ok = ((__ballot(!ok_pt) >> gbase) & 0xFull) == 0;
    // Newton divided differences -> monomial coefficients of the cubic (the
    // node spacings' reciprocals are constants: multiplies, not fp64
    // divisions -- q is an approximation whose own error the bound below
    // measures, so its last bits are free)
    const double d01 = (f1 - f0) * i10, d12 = (f2 - f1) * i21, d23 = (f3 - f2) * i32;
    const double d012 = (d12 - d01) * i20, d123 = (d23 - d12) * i31;
    const double d0123 = (d123 - d012) * i30;
    const double c3 = d0123;
    const double c2 = d012 - d0123 * (nd0 + nd1 + nd2);
    const double c1 = d01 - d012 * (nd0 + nd1) + d0123 * (nd0 * nd1 + nd0 * nd2 + nd1 * nd2);
    const double c0 = f0 - d01 * nd0 + d012 * nd0 * nd1 - d0123 * nd0 * nd1 * nd2;
    const float4 q = make_float4((float)c0, (float)c1, (float)c2, (float)c3);
    // the bound of |f^ - q| on this lane's sub-interval
    const double q0 = q.x, q1 = q.y, q2 = q.z, q3 = q.w;
    bool fail = !nodes_ok || !(off == off) || !isfinite(q0) || !isfinite(q1) || !isfinite(q2) ||
                !isfinite(q3);
    double bound = INFINITY;
    if (!fail) {
      double pbv[kP], pav[kP], lb[kLogD + 1], la[kLogD + 1], lnb = 0.0, lna = 0.0, rb = 0.0,
             ra = 0.0;
      cell_coefs(cell, 0, pbv);
      cell_coefs(cell, 1, pav);
      const bool okb = log_taylor(pbv, cI, r, lnb, lb, rb);
      const bool oka = log_taylor(pav, cI, r, lna, la, ra);
      if (okb && oka) {
        // the cubic's Taylor coefficients at cI
        const double qc = ((q3 * cI + q2) * cI + q1) * cI + q0;
        const double qk[4] = {qc, (3.0 * q3 * cI + 2.0 * q2) * cI + q1, 3.0 * q3 * cI + q2, q3};
        const double E0 = off + lnb - lna - qc;
        double sum = fabs(E0), rk = 1.0;
#pragma unroll
        for (int k = 1; k <= kLogD; ++k) {
          rk *= r;
          const double Ek = lb[k] - la[k] - (k < 4 ? qk[k] : 0.0);
          sum = fma(fabs(Ek), rk, sum);
        }
        // fp64 rounding of the whole computation (magnitudes ~|off| + |ln T0|)
        const double slack = 1e-13 * (1.0 + fabs(off) + fabs(lnb) + fabs(lna) + fabs(qc));
        bound = sum + rb + ra + slack;
      }
    }
    // the cell's bound: the largest of its 8 lanes'
    float bmax = (float)(bound * (1.0 + 1e-6));
#pragma unroll
    for (int o = 1; o < kScoreLanes; o <<= 1) bmax = fmaxf(bmax, __shfl_xor(bmax, o, kWave));
    if (!(bmax == bmax)) bmax = INFINITY;
    fail = fail || !(bmax <= (float)kFitTol);
    const bool bad = ((__ballot(fail) >> gbase) & ((1ull << kScoreLanes) - 1)) != 0;
    if (l == 0) {
      outs[c] = bad ? make_float4(__int_as_float(0x7FC00000), 0.0f, 0.0f, 0.0f) : q;
      if (bad && stats) atomicAdd(stats + 2, 1ull);
      if (!bad) {
        // |q'(u)| <= |c1| + 2|c2||u| + 3|c3|u^2 on |u| <= 1.0501
        const float sl = fabsf(q.y) + 2.11f * fabsf(q.z) + 3.31f * fabsf(q.w);
        slope = fmaxf(slope, sl);
        const float ev = 0x1.0p-21f * (1.0501f * fabsf(q.y) + 1.1028f * fabsf(q.z) +
                                        1.1581f * fabsf(q.w));
        const float ec = bmax + ev + (4.5f * 0x1.0p-24f + du_lg) * sl +
                         0x1.0p-24f * 1.0001f * (float)fabs(off);
        epsc = fmaxf(epsc, ec * 1.0001f);
      }
    }
  }
  slope = block_max<kBS, float>(slope, fred);
  epsc = block_max<kBS, float>(epsc, fred);
  // non-negative floats order as their bits
  if (threadIdx.x == 0 && slope > 0.0f)
    atomicMax(reinterpret_cast<unsigned int*>(&tables[blockIdx.y].slope), __float_as_uint(slope));
  if (threadIdx.x == 0 && epsc > 0.0f)
    atomicMax(reinterpret_cast<unsigned int*>(&tables[blockIdx.y].eps_cubic),
              __float_as_uint(epsc));
}

#ifndef TPE_BUILD_WPE  // diagnostic builds: waves-per-EU target of the build kernel
#define TPE_BUILD_WPE 1
#endif
__global__ __launch_bounds__(kBS) __attribute__((amdgpu_waves_per_eu(TPE_BUILD_WPE))) void k_table_build(
    const tpe_job* __restrict__ jobs, const tpe_seg* __restrict__ segs,
    const double* __restrict__ sigma, const double* __restrict__ coef64,
    const double* __restrict__ reach_hi, const double* __restrict__ reach_lo,
    const int32_t* __restrict__ wide_idx, tpe_table* __restrict__ tables,
    float* __restrict__ cells, unsigned long long* __restrict__ stats) {
  const tpe_job J = jobs[blockIdx.y];
  const tpe_table Tb = tables[blockIdx.y];
  const tpe_seg SB = segs[J.below], SA = segs[J.above];
  static_assert(kRefineCells <= kCoopCells, "a refined grid builds cooperatively");
  const Grid g = grid_of(Tb, J.tbl_cap, SB.n_obs + SA.n_obs + 2);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    tpe_table* W = tables + blockIdx.y;
    W->origin = g.origin;
    W->h = g.h;
    W->inv_h = (float)(1.0 / g.h);
    W->inv_w = (float)(0.5 / g.h);
    W->nb = g.nb;
    W->slope = 0.0f;  // raised by k_table_score (the next launch)
  }
  // (wid as a scalar: the quad, its cells' numbers and the span's ends are
  // wave-uniform and stay in scalar registers)
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), row = lane_id() >> 4;
  float* region = cells + J.tbl_off * (kSlotB / 4);
  __shared__ BuildLds X;
  // four consecutive cells (a "quad", one per 16-lane row) per wave; a label
  // with few cells (wide windows: many components per cell) gives each quad
  // the whole block, whose four waves split the components -- so it still
  // spreads over many waves when it is one of a rank's few labels
  const bool coop = g.nb <= kCoopCells;  // block-uniform
  const int64_t q0 = coop ? blockIdx.x : (int64_t)blockIdx.x * (kBS / kWave) + wid;
  const int64_t qs = coop ? gridDim.x : (int64_t)gridDim.x * (kBS / kWave);
  int itm = 0;       // most items a cell of this wave summed
  for (int64_t q = q0; 4 * q < g.nb; q += qs) {
    const int c0 = (int)(4 * q), c1 = min(c0 + 3, g.nb - 1);
    const int c = c0 + row;
    const bool mine = c < g.nb;
    const double y0 = (double)cell_centre((float)g.origin, (float)g.h, min(c, c1));
    const double ylo = (double)cell_centre((float)g.origin, (float)g.h, c0) - g.h;
    const double yhi = (double)cell_centre((float)g.origin, (float)g.h, c1) + g.h;
    float* out = region + (int64_t)min(c, c1) * kCellF;
    double mb, ma;
    const Windows w = cell_windows(SB, SA, reach_hi, reach_lo, ylo, yhi);
    const bool bb = build_mix(SB, coef64, w.lo_b, w.end_b - 1, wide_idx, Tb.n_wide_below,
                              Tb.T_below, y0, g.h, out, mine, 0, mb, X, coop, itm);
    const bool ba = build_mix(SA, coef64, w.lo_a, w.end_a - 1, wide_idx, Tb.n_wide_above,
                              Tb.T_above, y0, g.h, out, mine, 1, ma, X, coop, itm);
    if ((!coop || wid == 0) && (lane_id() & 15) == 0 && mine) {
      // dword 15: the score offset m_below - m_above, NaN marks a failed cell
      out[15] = (bb || ba) ? __int_as_float(0x7FC00000) : (float)(mb - ma);
      float* mp = region + (int64_t)J.tbl_cap * kCellF + 2 * c;  // (m_below, m_above)
      mp[0] = (float)mb;
      mp[1] = (float)ma;
      if ((bb || ba) && stats) atomicAdd(stats + 1, 1ull);
    }
  }
  // the job's worst case for the polynomial bound (mix_eps, k_table_score):
  // one atomic per wave (itm is wave-uniform)
  if (lane_id() == 0 && itm > 0) atomicMax(&tables[blockIdx.y].build_items, itm);
}
}  // namespace

void launch_table_plan(const tpe_job* jobs, int n_jobs, const tpe_seg* segs, const double* mu,
                       const double* sigma, const double* coef64, int max_comp, double* reach_hi,
                       double* reach_lo, int32_t* wide_idx, double* scratch, tpe_table* tables,
                       double draw_z, double tau, hipStream_t st) {
  const dim3 pg((max_comp + kBS - 1) / kBS, 2 * n_jobs);
  hipLaunchKernelGGL(k_table_plan1, pg, dim3(kBS), 0, st, jobs, segs, mu, sigma, coef64, reach_hi,
                     reach_lo, scratch, tables, draw_z, tau);
  hipLaunchKernelGGL(k_table_plan2, pg, dim3(kBS), 0, st, jobs, segs, mu, sigma, coef64, reach_hi,
                     reach_lo, wide_idx, scratch, tables);
}
}  // namespace tpe

using namespace tpe;

extern "C" int64_t tpe_table_scratch_bytes(int n_jobs, int max_comp) {
  if (n_jobs < 0 || max_comp < 0) return -1;
  const int64_t tiles = std::max(1, (max_comp + kBS - 1) / kBS);
  return 8 * (int64_t)kPlanStride * tiles * 2 * std::max(n_jobs, 1);
}

extern "C" int tpe_table_build(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                               const tpe_seg* segs, const double* mu, const double* sigma,
                               const double* coef64, int max_comp, double* reach_hi,
                               double* reach_lo, int32_t* wide_idx, double* scratch,
                               tpe_table* tables, float* cells, uint64_t* stats, void* stream) {
  bool inj = false;
  if (!check_gmm_jobs("tpe_table_build", host_jobs, n_jobs, 65535, kJobTable, &inj))
    return TPE_E_ARG;
  if (n_jobs == 0) return TPE_OK;
  if (!jobs || !segs || !mu || !sigma || !coef64 || !reach_hi || !reach_lo || !wide_idx ||
      !scratch || !tables || !cells) {
    set_error("tpe_table_build: null pointer");
    return TPE_E_ARG;
  }
  if (max_comp < 1 || n_jobs > 32767) {
    set_error("tpe_table_build: max_comp=%d n_jobs=%d", max_comp, n_jobs);
    return TPE_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  launch_table_plan(jobs, n_jobs, segs, mu, sigma, coef64, max_comp, reach_hi, reach_lo, wide_idx,
                    scratch, tables, kDrawZ, kTauExtra, st);
  hipLaunchKernelGGL(k_table_build, dim3(kBuildBlocks, n_jobs), dim3(kBS), 0, st, jobs, segs,
                     sigma, coef64, reach_hi, reach_lo, wide_idx, tables, cells,
                     (unsigned long long*)stats);
  int64_t cap = 1;
  for (int i = 0; i < n_jobs; ++i) cap = std::max(cap, host_jobs[i].tbl_cap);
  const int64_t sblocks =
      std::min<int64_t>(kScoreBlocks, (cap + kScoreCellsPerBlock - 1) / kScoreCellsPerBlock);
  hipLaunchKernelGGL(k_table_score, dim3((unsigned)sblocks, n_jobs), dim3(kBS), 0, st, jobs, tables,
                     cells, (unsigned long long*)stats);
  return check_launch("tpe_table_build");
}
