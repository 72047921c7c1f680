// tpe_table.hpp -- cell-table scoring of unquantized continuous labels: the
// method, the cell layout and what the table's translation units share
// (tpe_table.hip, tpe_table_score.hip, tpe_band.hip, tpe_pruned64.hip).
//
// Computes the same per-candidate quantities as GMM1_lpdf / LGMM1_lpdf
// (hyperopt/tpe.py:117-180, 265-307, logsum_rows :260-262) and the argmax of
// broadcast_best (tpe.py:649-658), for candidates sampled from the below
// posterior (tpe.py:79-106, 229-257) -- but without a component loop per
// candidate.
//
// Expansion.  In the scoring coordinate y (x for GMM1, log x for LGMM1) a
// mixture's density is S(y) = sum_j exp(l_j(y)),
//     l_j(y) = lc_j - 0.5 ((y - mu_j) inv_j)^2        (coef64: {mu, inv, lc, w}).
// The candidate range is cut into nb cells of half-width h.  Around a cell
// centre y0, with u = (y - y0)/h in [-1, 1],
//     l_j(y0 + h u) = l_j(y0) + A_j u + B_j u^2,
//     A_j = -h (y0 - mu_j) inv_j^2,   B_j = -0.5 h^2 inv_j^2,
// and exp(A u + B u^2) = sum_n c_n u^n with c_0 = 1, c_1 = A,
// (n+1) c_{n+1} = A c_n + 2B c_{n-1}.  So on the cell
//     S(y) = exp(m) * sum_{n<kP} P_n u^n,  P_n = sum_j exp(l_j(y0) - m) c_n^(j),
// a degree-8 polynomial per cell and mixture: the per-candidate work is two
// Horner evaluations and two logs, independent of the number of components.
//
// Error.  Every term is positive, so the relative error of S is at most the
// worst relative error of one component's truncated series.  |c_n| is at most
// the coefficient c~_n of exp(|A|u + |B|u^2) (same recurrence, all terms
// positive), so for |u| <= 1.05 the truncation error is at most
// e^{a+b} sum_{n>=9} c~_n 1.05^n (a = 1.05|A|, b = 1.05^2|B|); over
// 9|A| + 65|B| <= 5.8 its maximum is 4.3e-7.  P_0..P_5 are stored in fp32 and
// P_6..P_8 in fp16 (|P_n| <= e^{a+b} c~_n P_0, P_0 >= 1): the rounding adds at
// most 1.4e-7; the scorer evaluates that fp16 tail in fp16 arithmetic, which
// adds at most 4.4e-7 (tools/table_bounds.py 9 evaluates the three maxima).
// Components whose largest term anywhere in the candidate range is below
// exp(-tau)/M of the prior component's smallest term there (a lower bound of S
// everywhere) are left out: at most M of them, so together < exp(-tau) of S --
// 4.2e-8 at the table's tau = 17 (TPE_TAU_TABLE, tpe_table.hip), which mix_eps
// charges; the rest are found per cell through reach windows over the sorted
// means.
// The plan step chooses h so that every component that can be included in
// any cell satisfies the bound; if the cell budget (job.tbl_cap) forces a
// larger h, failing cells are flagged and their candidates take the exact
// fp32 log-sum-exp over all components.  Candidates outside the grid
// (injected values, rounding at the edges) take the exact path too.
//
// Layout.  One tpe_table per job plus a 128-B slot per cell: the job's region
// holds tbl_cap 64-B cells (four 16-B chunks, the scorer's whole gather), then
// tbl_cap (m_below, m_above) fp32 pairs (per-candidate outputs only):
//     floats [2n], [2n+1]: below / above P_n, n < 6                  chunks 0-2
//     dword 12 + (n - 6): fp16 {below P_n (low half), above P_n}, n = 6..8
//     [15] m_below - m_above (the score offset); NaN marks a cell that failed
//          the bound                                                  chunk 3
// The cell centre is not stored: both sides form it from the cell index
// (cell_centre).  The pairs (below P_n, above P_n) sit in adjacent registers
// for packed-FP32 Horner.
#pragma once

#include <algorithm>

#include "tpe_common.hpp"
#include "tpe_sample.hpp"

namespace tpe {
namespace {
constexpr int kP = 9;                // expansion terms per cell and mixture
constexpr int kP32 = 6;              // of which stored in fp32 (the rest in fp16)
constexpr int kCellF = 16;           // floats per cell (64 B: four 16-B chunks)
constexpr int kSlotB = 128;          // bytes per cell slot of a job's region (cells + m pairs)
constexpr int kChunks = 4;           // 16-B chunks of a cell the scorer reads
constexpr float kULim = 1.05f;       // |u| accepted by the scorer (fp32 cell-centre rounding)
#ifndef TPE_TRF
#define TPE_TRF 32
#endif
constexpr int kTRF = TPE_TRF;        // candidates per thread in the fast scorer (tpe_score_table_fast;
                                     // 32: its per-block setup and band tail over 8192 candidates --
                                     // 0.288 -> 0.272 ms per C3 level against 16, one-box A/B)
constexpr int64_t kTileF = (int64_t)kBS * kTRF;  // its tile: one band tile per scorer block

__device__ __forceinline__ double4 ld4(const double* coef64, int64_t k) {
  return reinterpret_cast<const double4*>(coef64)[k];
}

// wide components (the prior, and any with sigma >= prior_sigma / 4) are not
// windowed but listed; decided from the coefficient's 1/sigma everywhere
// (plan and build agree by construction)
__device__ __forceinline__ bool is_wide(const tpe_seg& S, int k, double inv) {
  return (k == S.prior_pos) || (inv <= 4.0 / S.prior_sigma);
}

// cell geometry from the plan (identical in every thread that asks)
struct Grid {
  double origin, h;
  int nb;
};

// centre of cell c in fp32 from the fp32 origin and half-width (the build
// expands around exactly this point; the scorer recomputes it from the cell
// index with the same two operations)
__device__ __forceinline__ float cell_centre(float origin, float h, int c) {
  return fmaf((float)(2 * c + 1), h, origin);
}
// A small job's grid is refined: the score cubic's error falls with h^4, and
// on the cells that the series bound alone admits a below mixture of a few
// components against a few hundred leaves 5-17 % of the sampler's mass (44 %
// for a 3-trial history) on cells whose cubic misses kFitTol -- those
// candidates then take the two-polynomial cell.  The build costs cells x
// components, so a job of at most kRefineComps components (both mixtures)
// gets up to kRefine times the cells the series bound asks for, never past
// kRefineCells (it stays a cooperative build) nor the job's budget.  Larger
// jobs (C3: 10^4 components) keep their grid.
constexpr int kRefine = 4;
constexpr int kRefineComps = 1024;
constexpr int kRefineCells = 4096;
__device__ __forceinline__ Grid grid_of(const tpe_table& Tb, int64_t cap, int n_comp) {
  const double span = Tb.hi - Tb.lo;
  double hn = fmin(Tb.h_below, Tb.h_above);
  if (!(hn > 0.0) || !isfinite(hn)) hn = fmax(span, 1.0);
  Grid g;
  if (!(span > 0.0)) {
    g.nb = 1;
    g.h = hn;
    g.origin = Tb.lo - hn;
    return g;
  }
  double n = ceil(span / (2.0 * hn));
  if (n_comp <= kRefineComps && n < (double)kRefineCells)
    n = fmin(n * (double)kRefine, (double)kRefineCells);
  if (!(n <= (double)cap)) n = (double)cap;
  g.nb = (int)fmax(1.0, n);
  g.h = span / (2.0 * g.nb);
  g.origin = Tb.lo;
  return g;
}

// first k with a[k] >= v / last k with a[k] <= v  (a non-decreasing)
__device__ __forceinline__ int first_ge(const double* a, int n, double v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] >= v) hi = mid; else lo = mid + 1;
  }
  return lo;
}
__device__ __forceinline__ int last_le(const double* a, int n, double v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] > v) hi = mid; else lo = mid + 1;
  }
  return lo - 1;
}

// The LGMM1 candidate drawn as y (fp32) is returned as x = exp(y) in fp64
// (cand_value), and the reference scores log(x) (tpe.py:284-287 via
// lognormal_lpdf, :208-217), which differs from y by the two roundings:
// |log(exp(y)) - y| <= 2^-51 (1 + |y|).  In cell units (|y| <= max(|lo|, |hi|)
// on the grid) that is a shift of u by at most this; the error bounds add it
// times the slope (the cubic's, or |P'| of the two-polynomial cell), so the
// band holds the winner of the scores at log(x).  0 for GMM1.
__host__ __device__ inline float lgmm_du(const tpe_job& J, const tpe_table& T) {
  if (J.family != TPE_LGMM1 || !(T.h > 0.0)) return 0.0f;
  const double ym = fmax(fabs(T.lo), fabs(T.hi)) + 2.0 * T.h;
  return (float)(0x1.0p-51 * (1.0 + ym) / T.h * 1.01);
}

__device__ __forceinline__ const float4* score_cells_of(const char* region, int64_t cap) {
  return reinterpret_cast<const float4*>(region + ((cap * (int64_t)(kCellF * 4 + 8) + 15) & ~15ll));
}

// the value of an unquantized candidate drawn as y in fp32: y (GMM1) or
// exp(y) evaluated in fp64 (LGMM1)
__device__ __forceinline__ double cand_value(float y, bool lgmm) {
  return lgmm ? exp((double)y) : (double)y;
}
// the coordinate its exact fp64 score is taken at: the returned value (GMM1)
// or log of it (LGMM1: the reference scores log(x) of the value it returns,
// tpe.py:284-287 / lognormal_lpdf :208-217) -- within lgmm_du of y in cell units
__device__ __forceinline__ double score_coord(float y, bool lgmm) {
  return lgmm ? log(cand_value(y, true)) : (double)y;
}

// Band tiles: every scorer block (tile of kTile candidates) writes a header
// {lo, hi_max, n} into band_ctl and its band entries into its own kTileSlots
// slots -- plain stores, no atomics (one returning atomic per block on a job
// word contended when a job's ~10^3 blocks ran together).  lo = the tile's
// best lower bound s - eps (a lower bound of G), hi_max = its largest upper
// bound (+inf with a NaN or log-sum-exp candidate), entries = its candidates
// with s + eps >= lo (a superset of the band's: G >= lo); a tile with more
// than kTileSlots such candidates writes n = kTileFull and no entries.
constexpr int kTileSlots = 256;  // (a plateau of near-equal scores puts ~60 of a tile's 4096
                                  // candidates in the band; 256 keeps such levels exact without
                                  // the whole-stream fp64 fallback)
constexpr uint32_t kTileFull = 0xFFFFFFFFu;
constexpr int kHdrWords = 4;  // per tile: lo, hi_max (float bits), n, unused

// scorer blocks (tiles) per job of the fast path: the partial layout
inline int64_t tpe_table_fast_tiles(const tpe_job* hj, int n) { return tiles_per_job(hj, n, kTileF); }
}  // namespace

// The plan (k_table_plan1/2, tpe_table.hip) of n_jobs jobs' mixtures of
// at most max_comp components: range, floors, reach windows and wide lists
// for draws within draw_z sigma and the exclusion margin tau.  scratch:
// tpe_table_scratch_bytes.
void launch_table_plan(const tpe_job* jobs, int n_jobs, const tpe_seg* segs, const double* mu,
                       const double* sigma, const double* coef64, int max_comp, double* reach_hi,
                       double* reach_lo, int32_t* wide_idx, double* scratch, tpe_table* tables,
                       double draw_z, double tau, hipStream_t st);
}  // namespace tpe
