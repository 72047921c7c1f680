// tpe_table_score.hip -- the two cell-table scorers.
//
// The per-candidate GMM1_lpdf / LGMM1_lpdf values (hyperopt/tpe.py:117-180,
// 265-307) and the argmax of broadcast_best (tpe.py:649-658) read from the
// cell table (tpe_table.hpp): k_score_table evaluates the two stored
// polynomials, k_score_table_fast the cell's cubic, leaving the candidates
// whose fp32 score could still win in the band (tpe_band.hip).
//
// Exports: tpe_table_partials, tpe_score_table, tpe_score_table_fast.
#include "tpe_table.hpp"

namespace tpe {
namespace {
#ifndef TPE_SCORE_WPE  // waves per SIMD the fast scorer is compiled for (its VGPR budget;
#define TPE_SCORE_WPE 4  // its 32 KB draw stage per block allows four blocks per CU anyway)
#endif
#ifndef TPE_TR
#define TPE_TR 16
#endif
constexpr int kTR = TPE_TR;          // candidates per thread and tile in the scorer
#ifndef TPE_TILES
#define TPE_TILES 1
#endif
constexpr int kTiles = TPE_TILES;    // tiles (kBS * kTR candidates) per scorer block
constexpr int64_t kTile = (int64_t)kBS * kTR;
constexpr float kLn2T = 0.6931471805599453f;

// ---------------------------------------------------------------------------
// scoring
// ---------------------------------------------------------------------------
typedef float f4 __attribute__((ext_vector_type(4)));  // native vector (no memcpy copies)

// f(integral_constant<int, R>) for R = B .. E-1, unrolled at compile time
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}

// both mixtures' degree-8 polynomials at u: q0..q2 = fp32 pairs
// (b_2k, a_2k, b_2k+1, a_2k+1), q3 = fp16 pairs {b_n | a_n} for n = 6..8 (and
// the score offset in q3.w).  The fp16 tail P_6 + u(P_7 + u P_8) is evaluated
// in packed fp16 (v_pk_fma_f16, both mixtures per instruction; its rounding is
// bounded in tools/table_bounds.py), the fp32 steps are packed FMAs
// (v_pk_fma_f32) on adjacent registers
typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void horner9x2(const f4 q0, const f4 q1, const f4 q2, const f4 q3,
                                          float u, float& pb, float& pa) {
  static_assert(kP == 9 && kP32 == 6, "six fp32 and three fp16 terms");
  const h2_t c6 = __builtin_bit_cast(h2_t, q3.x), c7 = __builtin_bit_cast(h2_t, q3.y),
             c8 = __builtin_bit_cast(h2_t, q3.z);
  const _Float16 uh = (_Float16)u;
  const h2_t uu = {uh, uh};
  h2_t t = __builtin_elementwise_fma(c8, uu, c7);
  t = __builtin_elementwise_fma(t, uu, c6);
  float b = (float)t.x, a = (float)t.y;
#define TPE_H2(cb, ca) b = fmaf(b, u, cb); a = fmaf(a, u, ca);
  TPE_H2(q2.z, q2.w) TPE_H2(q2.x, q2.y) TPE_H2(q1.z, q1.w) TPE_H2(q1.x, q1.y)
  TPE_H2(q0.z, q0.w) TPE_H2(q0.x, q0.y)
#undef TPE_H2
  pb = b;
  pa = a;
}

// exact fp32 log-sum-exp over every component (natural log), the dense
// kernel's arithmetic: t = xc*a + b, v = c - t^2 in log2 units offset by cmax
__device__ __forceinline__ float lse_exact32(const float4* __restrict__ coef, const tpe_seg& S, float y) {
  const float xc = y - (float)S.center;
  float m = -INFINITY, s = 0.0f;
#pragma unroll 8
  for (int k = 0; k < S.n_obs + 1; ++k) {
    const float4 c = coef[k];
    const float t = fmaf(xc, c.x, c.y);
    const float v = fmaf(-t, t, c.z);
    if (v > m) {
      s = s * __builtin_amdgcn_exp2f(m - v) + 1.0f;
      m = v;
    } else {
      s += __builtin_amdgcn_exp2f(v - m);
    }
  }
  return (m + __builtin_amdgcn_logf(s) + (float)S.cmax) * kLn2T;
}

// The same log-sum-exp with the whole wave on one candidate (y wave-uniform,
// every lane active): lane l sums components l, l + 64, ... online, then the
// 64 partial sums are merged at the wave's maximum.  A per-lane serial sum over
// 10^4 components is ~10^5 instructions in one lane -- a tail of ~100 us for
// the wave that holds such a candidate.  Rounding: <= M/64 + 8 sequential
// steps per term, inside the bound taken for the serial sum (kEpsLse).
__device__ __forceinline__ float lse_wave32(const float4* __restrict__ coef, const tpe_seg& S,
                                            float y) {
  const float xc = y - (float)S.center;
  float m = -INFINITY, s = 0.0f;
  for (int k = lane_id(); k < S.n_obs + 1; k += kWave) {
    const float4 c = coef[k];
    const float t = fmaf(xc, c.x, c.y);
    const float v = fmaf(-t, t, c.z);
    if (v > m) {
      s = s * __builtin_amdgcn_exp2f(m - v) + 1.0f;
      m = v;
    } else {
      s += __builtin_amdgcn_exp2f(v - m);
    }
  }
  float M = m;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) M = fmaxf(M, __shfl_xor(M, o, kWave));
  float t = (m == -INFINITY) ? 0.0f : s * __builtin_amdgcn_exp2f(m - M);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) t += __shfl_xor(t, o, kWave);
  return (M + __builtin_amdgcn_logf(t) + (float)S.cmax) * kLn2T;
}

template <bool INJ>
__global__ __launch_bounds__(kBS) void k_score_table(
    const tpe_job* __restrict__ jobs, const tpe_seg* __restrict__ segs,
    const double* __restrict__ mu, const double* __restrict__ sigma,
    const double* __restrict__ wcdf, const float4* __restrict__ coef32,
    const tpe_table* __restrict__ tables, const float* __restrict__ cells,
    const double* __restrict__ cand, double* __restrict__ out_bl, double* __restrict__ out_al,
    double* __restrict__ out_x, tpe_best* __restrict__ partial,
    unsigned long long* __restrict__ stats, int n_tiles, int n_jobs) {
  __shared__ MixLds s_mix;
  // per wave: 4 DMA slabs of 64 x 16 B, the gather's LDS image; also the
  // sampler's staging buffer before scoring
  __shared__ float4 s_rows[(kBS / kWave) * kWave * kChunks];
  __shared__ uint16_t s_list[(kBS / kWave) * kRetryList];
  __shared__ BestT red[kBS / kWave];
  __shared__ int nred[kBS / kWave];
  static_assert(kTR * kWave * sizeof(float) <= kWave * kChunks * sizeof(float4), "staging alias");
  // XCD-aware work order: consecutive blocks land on consecutive XCDs (block
  // b on XCD b % 8), so block b takes work item (b % 8) * per + b / 8 of the
  // (job, tile) list -- each XCD sweeps one contiguous eighth of it and its
  // L2 holds the cell tables of ~1/8 of the labels instead of all of them
  int job, bx;
  {
    const int64_t W = (int64_t)n_tiles * n_jobs, per = (W + 7) / 8;
    const int64_t w = (int64_t)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
    if (w >= W) return;  // padding block (the grid is 8 * per)
    job = (int)(w / n_tiles);
    bx = (int)(w - (int64_t)job * n_tiles);
  }
  const tpe_job J = jobs[job];
  tpe_best* P = partial + (int64_t)job * n_tiles + bx;
  const int64_t base0 = (int64_t)bx * kTiles * kTile;
  if (base0 >= J.n_cand) {
    if (threadIdx.x == 0) *P = empty_best();
    return;
  }
  const tpe_seg SB = segs[J.below], SA = segs[J.above];
  const tpe_table Tb = tables[job];
  const bool lgmm = J.family == TPE_LGMM1;
  const bool lo_on = J.flags & TPE_F_LOW, hi_on = J.flags & TPE_F_HIGH;
  const bool log_in = INJ && lgmm, exp_out = !INJ && lgmm;
  const float g0 = (float)Tb.origin, inv_w = Tb.inv_w, inv_h = Tb.inv_h;
  const int nb = Tb.nb;
  // the job's cell table: a uniform base + 32-bit byte offsets (saddr loads)
  const char* cbase = reinterpret_cast<const char*>(cells) + J.tbl_off * kSlotB;
  const float* mpairs = reinterpret_cast<const float*>(cbase) + J.tbl_cap * kCellF;
  const float h32 = (float)Tb.h;
  const int lane = lane_id(), gi = lane & (kChunks - 1), gbase = lane & ~(kChunks - 1);
  // wave-uniform (scalar) base of the wave's LDS region: the DMA destinations need no
  // per-instruction readfirstlane
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  float4* rows = s_rows + wave * (kWave * kChunks);
  const bool outs = out_bl || out_al || out_x;
  Mix M{};
#ifndef TPE_DIAG_SKIP_SAMPLE
  if (!INJ) M = stage_mix(SB, wcdf, mu, sigma, s_mix);  // once per block
#endif
  BestT run{0.0, -1, 0.0};
  int n_exact = 0;
  // the block's tiles in index order; a thread owns kTR consecutive candidates
  // of each (pairs share a Philox call)
  for (int tile = 0; tile < kTiles; ++tile) {
    const int64_t base = base0 + tile * kTile;
    if (base >= J.n_cand) break;
    if (tile > 0) __syncthreads();  // the previous tile's slabs / stash are done
    const int64_t t0 = base + (int64_t)threadIdx.x * kTR;
    // x[r]: the candidate in the scoring coordinate y for sampled jobs (log x for
    // LGMM1; the value exp(y) is formed only for outputs and the winner), the
    // given value for injected ones
    float x[kTR];
    if (INJ) {
#pragma unroll
      for (int r = 0; r < kTR; ++r) x[r] = t0 + r < J.n_cand ? (float)cand[J.cand_off + t0 + r] : 1.0f;
    } else {
#ifdef TPE_DIAG_SKIP_SAMPLE  // diagnostic builds only (tools/probes/diag_variants.sh)
      const float w = 2.0f * (float)Tb.h * (float)Tb.nb;
#pragma unroll
      for (int r = 0; r < kTR; ++r)
        x[r] = (float)Tb.origin + w * __builtin_amdgcn_fractf((float)(t0 + r) * 0.6180339887f);
#else
      const int nv = (int)max((int64_t)0, min((int64_t)kTR, J.n_cand - t0));
      draw32_pairs<kTR>(M, J.key, J.cand_base + t0, nv, lo_on, hi_on, bound32(J.low),
                        bound32(J.high), false, reinterpret_cast<float*>(rows), s_list + (threadIdx.x / kWave) * kRetryList, x);
#endif
    }
    // per-thread argmax in fp32 over the thread's candidates r = 0..kTR-1
    // (np.argmax rules: larger score, NaN wins, ties -> smaller r)
    float bs = -INFINITY, by = 0.0f;
    int br = -1;
    uint32_t exact_mask = 0;
    auto outputs = [&](float lb, float la, float y, int r) {
      double bl = lb, al = la;
      if (lgmm) {  // lognormal_lpdf's -log(x) (tpe.py:214-216): in both, not in the score
        bl -= (double)y;
        al -= (double)y;
      }
      const int64_t o = J.out_off + t0 + r;
      if (out_bl) out_bl[o] = bl;
      if (out_al) out_al[o] = al;
      if (out_x) out_x[o] = exp_out ? exp((double)y) : (double)y;
    };
    const int nvalid = (int)max((int64_t)0, min((int64_t)kTR, J.n_cand - t0));
    // cell of every candidate of the thread (byte offset in the job's table)
    float yv[kTR];
    uint32_t co[kTR];
#pragma unroll
    for (int r = 0; r < kTR; ++r) {
      yv[r] = log_in ? __logf(x[r]) : x[r];
      const float t = (yv[r] - g0) * inv_w;
      int c = (t >= 0.0f) ? (int)t : 0;  // NaN -> 0
      co[r] = (uint32_t)min(c, nb - 1) * (kCellF * 4);
    }
    // Cooperative gather by LDS-DMA: lane gi of each 4-lane group fetches one
    // 16-B chunk of every group member's 64-B cell (global_load_lds_dwordx4),
    // so a wave-instruction touches 16 cells instead of 64 and the data lands
    // in LDS without passing through VGPRs.  Slab j holds member j's cells:
    // lane (g, gi) brings chunk gi^j, so lane (g, j) reads its chunk k from
    // slab j, slot 4g + (k^j) -- conflict-free ds_read_b128.  Candidate r+1's
    // DMA is issued as soon as candidate r's chunks are in registers, and runs
    // under r's polynomial work.
    typedef __attribute__((address_space(3))) void* lds_vp;
    typedef const __attribute__((address_space(1))) void* glb_vp;
    auto fetch = [&](int r) __attribute__((always_inline)) {
      auto one = [&](auto jc) __attribute__((always_inline)) {
        constexpr int j = decltype(jc)::value;
        // member j's cell offset: a quad-perm broadcast inside the 4-lane group
        const uint32_t cj = (uint32_t)__builtin_amdgcn_mov_dpp(
            (int)co[r], j | (j << 2) | (j << 4) | (j << 6), 0xF, 0xF, true);
        __builtin_amdgcn_global_load_lds((glb_vp)(cbase + (cj + ((gi ^ j) * 16))),
                                         (lds_vp)(rows + j * kWave), 16, 0, 0);
      };
      static_for<0, kChunks>(one);
    };
    const f4* slab = reinterpret_cast<const f4*>(rows) + gi * kWave;
    auto score = [&](auto rc) __attribute__((always_inline)) {
      constexpr int r = decltype(rc)::value;
      const float y = yv[r];
      // candidate r's DMA has landed (the compiler does not order LDS-DMA
      // writes before later ds_reads by itself)
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
      static_assert(kChunks == 4, "the reads below take chunks 0..3");
      const f4 q0 = slab[gbase | gi], q1 = slab[gbase | (1 ^ gi)], q2 = slab[gbase | (2 ^ gi)],
               q3 = slab[gbase | (3 ^ gi)];
      // the reads must land before the next candidate's DMA overwrites the slabs
      __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
      if constexpr (r + 1 < kTR) fetch(r + 1);
      const int cell = (int)(co[r] / (kCellF * 4));
      const float u = (y - cell_centre(g0, h32, cell)) * inv_h;
      float pb, pa;
      horner9x2(q0, q1, q2, q3, u, pb, pa);
      const float dlog = (__builtin_amdgcn_logf(pb) - __builtin_amdgcn_logf(pa)) * kLn2T;
      const bool valid = r < nvalid;
      // q3.w: m_below - m_above, NaN for a cell that failed the bound
      const bool ok = (q3.w == q3.w) && (fabsf(u) <= kULim) && (pb > 0.0f) && (pa > 0.0f);
      exact_mask |= (valid && !ok) ? (1u << r) : 0u;
      if (valid && ok) {
        if (outs)
          outputs(mpairs[2 * cell] + __builtin_amdgcn_logf(pb) * kLn2T,
                  mpairs[2 * cell + 1] + __builtin_amdgcn_logf(pa) * kLn2T, y, r);
        // table scores are finite: strict > keeps the first of equal scores
        const float sc = q3.w + dlog;
        const bool take = sc > bs;
        bs = take ? sc : bs;
        by = take ? (INJ ? x[r] : y) : by;
        br = take ? r : br;
      }
    };
#ifdef TPE_DIAG_SKIP_SCORE  // diagnostic builds only: the sampler alone
#pragma unroll
    for (int r = 0; r < kTR; ++r)
      if (t0 + r < J.n_cand && yv[r] > bs) {
        bs = yv[r];
        by = yv[r];
        br = r;
      }
#else
    fetch(0);
    static_for<0, kTR>(score);
#endif
    // exact fp32 log-sum-exp for the (rare) candidates the table does not cover;
    // their values wait in the lane's own LDS row
    if (__any(exact_mask != 0)) {
      float* stash = reinterpret_cast<float*>(rows + lane * (kTR / 4));
#pragma unroll
      for (int r = 0; r < kTR; ++r)
        if (exact_mask & (1u << r)) stash[r] = x[r];
      __builtin_amdgcn_wave_barrier();
      while (exact_mask) {
        const int r = __builtin_ctz(exact_mask);
        exact_mask &= exact_mask - 1;
        const float xv = stash[r];
        const float y = log_in ? __logf(xv) : xv;
        const float lb = lse_exact32(coef32 + SB.comp_off, SB, y);
        const float la = lse_exact32(coef32 + SA.comp_off, SA, y);
        if (outs) outputs(lb, la, y, r);
        const float sc = lb - la;
        const bool na = sc != sc, nb_ = bs != bs;
        const bool take =
            (br < 0) || (na ? (!nb_ || r < br) : (!nb_ && (sc > bs || (sc == bs && r < br))));
        if (take) {
          bs = sc;
          br = r;
          by = INJ ? xv : y;
        }
        ++n_exact;
      }
    }
    // the winner's value (by: the given value, or y of a sampled candidate --
    // exp(y) in fp64 for LGMM1, the value every fp32 scorer gives)
    const double bx = exp_out ? exp((double)by) : (double)by;
    if (br >= 0) best_update(run, (double)bs, J.cand_base + t0 + br, bx);
  }  // tiles
  const BestT best = block_best<kBS>(run, red);
  if (stats) {
    const int ne = block_sum<kBS, int>(n_exact, nred);
    if (threadIdx.x == 0 && ne) atomicAdd(stats, (unsigned long long)ne);
  }
  if (threadIdx.x == 0) *P = tpe_best{best.score, best.index, best.value, 0};
}

// fp32 score error bound of the fast path.  A candidate
// scored by its cell's cubic has
//     |s32 - s64| <= eps_cubic + 2.0001 eps_mix + 2^-22 |s32|
// (tpe_table: eps_cubic bounds the cubic against the stored polynomials, its
// fp32 evaluation beyond the |s| part, u's rounding and the fp32 offset;
// eps_mix the stored polynomial against its mixture, whose log then moves by
// at most eps_mix / (1 - eps_mix)).  A candidate of the two-polynomial cell
// carries its own bound (eps_2poly); one of the exact fp32 log-sum-exp
// fallback is always re-scored in fp64 (its hi is +inf).
constexpr float kEpsRel = 0x1.0p-22f;  // >= gamma_3 of the cubic's three fp32 FMAs

// outward rounding of a round-to-nearest fp32 result x (|exact - x| <= ulp/2
// <= 2^-24 |x|): up(x) >= exact >= dn(x) (the fma adds at least one ulp; the
// 1e-30 covers x = 0)
__device__ __forceinline__ float up(float x) { return fmaf(fabsf(x), 0x1.0p-23f, x) + 1e-30f; }
__device__ __forceinline__ float dn(float x) { return fmaf(-fabsf(x), 0x1.0p-23f, x) - 1e-30f; }
constexpr float kEtaLog2 = 0x1.0p-22f;  // v_log_f32 error, absolute or relative to |log2 p| (checked exhaustively)

// order-preserving float -> uint32 code (larger float, larger code; code 0 is
// below every float: "no value yet")
__device__ __forceinline__ uint32_t ord_enc(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ord_dec(uint32_t e) {
  if (e == 0u) return -INFINITY;
  return __uint_as_float((e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e);
}

// relative error bound of one mixture's two-polynomial value p (fp32 Horner
// from the fp16 tail, horner9x2) at u against the stored polynomial at the
// exact u: gamma_6 times the absolute polynomial, the fp16 tail's rounding
// (u to fp16, two fp16 FMAs, subnormal spacing), and u's fp32 rounding times
// a bound of |P'|; +inf when it is not below p
__device__ __forceinline__ float poly_rel_err(const float (&P)[kP], float u, float p, float du) {
  const float au = fabsf(u);
  float pabs = 0.0f, pd = 0.0f;
#pragma unroll
  for (int n = kP - 1; n >= 0; --n) {
    pabs = fmaf(pabs, au, fabsf(P[n]));
    if (n >= 1) pd = fmaf(pd, 1.0501f, (float)n * fabsf(P[n]));
  }
  const float dt = 0x1.0p-9f * 1.16f * (fabsf(P[6]) + fabsf(P[7]) + fabsf(P[8])) + 0x1.0p-23f;
  const float dp = (6.1f * 0x1.0p-24f * pabs + 1.35f * dt + du * pd) * 1.001f;
  return dp < p ? dp / (p - dp) : INFINITY;
}

// bound of |s - s64| for a two-polynomial score s = off + (lb2 - la2) ln2,
// beyond the polynomials' own 2.0001 eps_mix
__device__ __forceinline__ float eps_2poly(const f4 q0, const f4 q1, const f4 q2, const f4 q3,
                                           float u, float pb, float pa, float lb2, float la2,
                                           float s, float du) {
  float Pb[kP], Pa[kP];
  const float c[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
#pragma unroll
  for (int n = 0; n < kP32; ++n) {
    Pb[n] = c[2 * n];
    Pa[n] = c[2 * n + 1];
  }
  const h2_t t6 = __builtin_bit_cast(h2_t, q3.x), t7 = __builtin_bit_cast(h2_t, q3.y),
             t8 = __builtin_bit_cast(h2_t, q3.z);
  Pb[6] = (float)t6.x; Pa[6] = (float)t6.y;
  Pb[7] = (float)t7.x; Pa[7] = (float)t7.y;
  Pb[8] = (float)t8.x; Pa[8] = (float)t8.y;
  const float rb = poly_rel_err(Pb, u, pb, du), ra = poly_rel_err(Pa, u, pa, du);
  const float off = fabsf(q3.w);
  return (0x1.0p-24f * off + rb + ra +
          kLn2T * kEtaLog2 * (fmaxf(1.0f, fabsf(lb2)) + fmaxf(1.0f, fabsf(la2))) +
          0x1.0p-21f * (fabsf(s) + off + kLn2T * (fabsf(lb2) + fabsf(la2)))) * 1.001f;
}

// Fast path for sampled candidates (the suggest path: no per-candidate
// log-densities asked for).  Same draws as k_score_table (draw32_pairs), same
// cell index; the score comes from the cell's 16-B cubic (k_table_score):
// one global_load_dwordx4 per candidate instead of a 64-B gather, and three
// FMAs instead of two degree-8 polynomials and two logs.  Loads run four
// candidates ahead.  Candidates on a flagged score cell (or off the grid)
// take the two-polynomial cell, then the exact log-sum-exp, after the loop.
// out_score / out_x / out_eps (nullable, tests): per-candidate fp32 score,
// value and the bound eps the band used (+inf: always re-scored).
template <bool HOOKS>  // HOOKS: the per-candidate test outputs (out_score / out_x / out_eps)
__global__ __launch_bounds__(kBS) __attribute__((amdgpu_waves_per_eu(TPE_SCORE_WPE))) void k_score_table_fast(
    const tpe_job* __restrict__ jobs, const tpe_seg* __restrict__ segs,
    const double* __restrict__ mu, const double* __restrict__ sigma,
    const double* __restrict__ wcdf, const float4* __restrict__ coef32,
    const tpe_table* __restrict__ tables, const float* __restrict__ cells,
    tpe_band* __restrict__ band, uint32_t* __restrict__ band_ctl,
    double* __restrict__ out_score, double* __restrict__ out_x, double* __restrict__ out_eps,
    tpe_best* __restrict__ partial, unsigned long long* __restrict__ stats, int n_tiles,
    int n_jobs, int tile_cap) {
  __shared__ LeanMix s_lean;
  // retry staging, then each lane's scores (slot r of lane l at r * 64 + l)
  __shared__ float s_stage[(kBS / kWave) * kTRF * kWave];
  __shared__ uint16_t s_list[(kBS / kWave) * kRetryList];
  __shared__ uint64_t s_key[kBS / kWave];
  __shared__ float s_wy[kBS / kWave];
  __shared__ float s_lo[kBS / kWave], s_hi[kBS / kWave];
  __shared__ int s_cnt[kBS / kWave];
  __shared__ int s_n;
  int job, bx;
  {  // XCD-aware work order (see k_score_table)
    const int64_t W = (int64_t)n_tiles * n_jobs, per = (W + 7) / 8;
    const int64_t w = (int64_t)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
    if (w >= W) return;
    job = (int)(w / n_tiles);
    bx = (int)(w - (int64_t)job * n_tiles);
  }
  const tpe_job J = jobs[job];
  tpe_best* P = partial + (int64_t)job * n_tiles + bx;
  uint32_t* hdr = band_ctl + ((int64_t)job * n_tiles + bx) * kHdrWords;
  const int64_t base = (int64_t)bx * kTileF;
  if (base >= J.n_cand) {
    if (threadIdx.x == 0) {
      *P = empty_best();
      hdr[0] = __float_as_uint(-INFINITY);
      hdr[1] = __float_as_uint(-INFINITY);
      hdr[2] = 0u;
    }
    return;
  }
  const tpe_seg SB = segs[J.below], SA = segs[J.above];
  const tpe_table Tb = tables[job];
  const bool lgmm = J.family == TPE_LGMM1;
  const bool lo_on = J.flags & TPE_F_LOW, hi_on = J.flags & TPE_F_HIGH;
  const float g0 = (float)Tb.origin, inv_w = Tb.inv_w, inv_h = Tb.inv_h, h32 = (float)Tb.h;
  const int nb = Tb.nb;
  const char* region = reinterpret_cast<const char*>(cells) + J.tbl_off * kSlotB;
  const float4* sc = score_cells_of(region, J.tbl_cap);
  const int lane = lane_id();
  float* stage = s_stage + (threadIdx.x / kWave) * (kTRF * kWave);
  // the below mixture: staged for the lean sampler (tpe.suggest: always --
  // at most 26 components) or read from global memory (draw32_pairs)
  const int nmix = SB.n_obs + 1;
  const bool lean = nmix <= kStage;  // block-uniform
  const Mix M{wcdf + SB.comp_off, mu + SB.comp_off, sigma + SB.comp_off, nullptr, nullptr,
              nullptr, nmix};
  const int64_t t0 = base + (int64_t)threadIdx.x * kTRF;
  const int nvalid = (int)max((int64_t)0, min((int64_t)kTRF, J.n_cand - t0));
  const float lo32 = bound32(J.low), hi32 = bound32(J.high);
  uint16_t* wlist = s_list + (threadIdx.x / kWave) * kRetryList;
  // the candidates, in the scoring coordinate y (log x for LGMM1), into the
  // wave's stage (slot r of lane l at r * 64 + l)
  if (lean) {
    stage_lean(SB, wcdf, mu, sigma, s_lean);
    if (lo_on || hi_on)
      lean_draw<kTRF, true>(s_lean, nmix, J.key, J.cand_base + t0, nvalid, lo_on, hi_on, lo32,
                           hi32, stage, wlist);
    else
      lean_draw<kTRF, false>(s_lean, nmix, J.key, J.cand_base + t0, nvalid, false, false, lo32,
                            hi32, stage, wlist);
  } else {
    // a below mixture past the LDS staging (explicit observation lists, never
    // tpe.suggest's): one candidate at a time, the same stream (draw32)
#pragma unroll 1
    for (int r = 0; r < kTRF; ++r)
      stage[r * kWave + lane] =
          r < nvalid ? draw32(M, J.key, J.cand_base + t0 + r, lo_on, hi_on, lo32, hi32) : 1.0f;
  }
  // candidate g again, exactly as drawn above (the tile winner's and the band
  // entries' values: x[] need not live through the tail)
  auto redraw = [&](int64_t g) __attribute__((always_inline)) -> float {
    return lean ? lean_draw1(s_lean, nmix, J.key, g, lo_on, hi_on, lo32, hi32)
                : draw32(M, J.key, g, lo_on, hi_on, lo32, hi32);
  };
  const float nbm1 = (float)(nb - 1);
  // the cell of y: trunc of (y - origin) / 2h clamped to [0, nb - 1] (NaN -> 0)
  auto cell_of = [&](float y) __attribute__((always_inline)) -> int {
    return (int)__builtin_amdgcn_fmed3f((y - g0) * inv_w, 0.0f, nbm1);
  };
  auto cubic_at = [&](int c) __attribute__((always_inline)) -> float4 {
    return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(sc) +
                                            ((uint32_t)c << 4));
  };
  float bs = -INFINITY, by = 0.0f;
  int br = -1;
  uint32_t fb = 0;  // candidates the score cells do not cover
  // FULL: every slot of the thread valid (all but a job's last tile).  y is
  // read back from the stage four candidates ahead of its score, together
  // with its cell's cubic; the slot then takes the score (or, for a fallback
  // candidate, keeps y).  Branch-free: slots past the job's end are scored
  // like the rest and masked out of the argmax and the fallback mask.
  auto score_all = [&](auto full_tag) __attribute__((always_inline)) {
    constexpr bool FULL = decltype(full_tag)::value;
    float yq[4];
    float4 q[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      yq[r] = stage[r * kWave + lane];
      q[r] = cubic_at(cell_of(yq[r]));
    }
#pragma unroll
    for (int r = 0; r < kTRF; ++r) {
      const float y = yq[r & 3];
      const int c = cell_of(y);
      const float4 k = q[r & 3];
      if (r + 4 < kTRF) {
        yq[r & 3] = stage[(r + 4) * kWave + lane];
        q[r & 3] = cubic_at(cell_of(yq[r & 3]));
      }
#ifdef TPE_DIAG_SKIP_SCORE  // diagnostic builds only: the sampler alone (the draw is its score)
      const float s = y + 0.0f * (float)c + 0.0f * k.x;
      const bool ok = true;
#else
      const float u = (y - cell_centre(g0, h32, c)) * inv_h;
      const float s = fmaf(fmaf(fmaf(k.w, u, k.z), u, k.y), u, k.x);
      const bool ok = (s == s) && (fabsf(u) <= kULim);
#endif
      fb |= ok ? 0u : (1u << r);
      // finite scores: strict > keeps the first of equal scores (np.argmax)
      const float sv = (ok && (FULL || r < nvalid)) ? s : -INFINITY;
      const bool take = sv > bs;
      br = take ? r : br;
      by = take ? y : by;
      bs = fmaxf(bs, sv);
      // kept for the band (a fallback candidate keeps its y for the fallback pass)
      stage[r * kWave + lane] = ok ? s : y;
      if (HOOKS && out_score && ok && r < nvalid) out_score[J.out_off + t0 + r] = (double)s;
      if (HOOKS && out_x && r < nvalid) out_x[J.out_off + t0 + r] = cand_value(y, lgmm);
    }
    if (!FULL) fb &= nvalid <= 0 ? 0u : (1u << nvalid) - 1u;
  };
  if (nvalid == kTRF)
    score_all(std::true_type{});
  else
    score_all(std::false_type{});
  // the lane's best cubic-scored candidate (its bounds are monotone in s)
  const float bs_cubic = bs;
  const float ea = (Tb.eps_cubic + 2.0001f * Tb.eps_mix) * 1.000001f;  // (covers its rounding)
  // eps(s) = ea + 2^-22 |s| of a cubic-scored candidate; bounds s -/+ eps are
  // rounded outwards (up / dn)
  auto eps_of = [&](float v) __attribute__((always_inline)) -> float {
    return fmaf(kEpsRel, fabsf(v), ea) * 1.000001f;
  };
  float lo_fb = -INFINITY, hi_fb = -INFINITY;  // the lane's fallback candidates' bounds
  int n_fb = 0;
  uint32_t lsem = 0;  // candidates scored by the exact fp32 log-sum-exp
  const uint32_t fbm = fb;
  if (__any(fb != 0)) {
    // fallback: the two-polynomial cell, else the exact fp32 log-sum-exp;
    // the lane's candidates wait in its own column of the wave's stage, and
    // their UPPER BOUNDS (two-polynomial) or scores (log-sum-exp) replace
    // them there
    // (the fallback candidates' y were staged by their own lanes above; the
    // log-sum-exp below reads other lanes' columns)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const f4* cell4 = reinterpret_cast<const f4*>(region);
    auto fold = [&](int r, float s, float y, float keep) __attribute__((always_inline)) {
      stage[r * kWave + lane] = keep;
      if (HOOKS && out_score) out_score[J.out_off + t0 + r] = (double)s;
      const bool na = s != s, nbn = bs != bs;
      const bool take =
          (br < 0) || (na ? (!nbn || r < br) : (!nbn && (s > bs || (s == bs && r < br))));
      if (take) {
        bs = s;
        br = r;
        by = y;
      }
      ++n_fb;
    };
    while (fb) {
      const int r = __builtin_ctz(fb);
      fb &= fb - 1;
      const float y = stage[r * kWave + lane];
      const int c = cell_of(y);
      const float u = (y - cell_centre(g0, h32, c)) * inv_h;
      const f4 q0 = cell4[4 * c], q1 = cell4[4 * c + 1], q2 = cell4[4 * c + 2],
               q3 = cell4[4 * c + 3];
      float pb, pa;
      horner9x2(q0, q1, q2, q3, u, pb, pa);
      bool done = false;
      if ((q3.w == q3.w) && (fabsf(u) <= kULim) && (pb > 0.0f) && (pa > 0.0f) &&
          isfinite(pb) && isfinite(pa)) {
        const float lb2 = __builtin_amdgcn_logf(pb), la2 = __builtin_amdgcn_logf(pa);
        const float s = q3.w + (lb2 - la2) * kLn2T;
        const float e2 = eps_2poly(q0, q1, q2, q3, u, pb, pa, lb2, la2, s,
                                   4.5f * 0x1.0p-24f + lgmm_du(J, Tb)) +
                         2.0001f * Tb.eps_mix;
        if (s == s && e2 < INFINITY) {
          const float hi = up(s + e2);
          fold(r, s, y, hi);
          lo_fb = fmaxf(lo_fb, dn(s - e2));
          hi_fb = fmaxf(hi_fb, hi);
          if (HOOKS && out_eps) out_eps[J.out_off + t0 + r] = (double)hi - (double)s;
          done = true;
        }
      }
      if (!done) lsem |= 1u << r;  // the exact log-sum-exp, below, the wave together
    }
    // the exact fp32 log-sum-exp over every component, one candidate at a
    // time with the whole wave (its y still waits in the stage); always in
    // the band (hi = +inf: its bound is not tracked)
    uint32_t ex = lsem;
    for (;;) {
      const uint64_t lanes = __ballot(ex != 0);
      if (!lanes) break;
      const int L = __builtin_ctzll(lanes);
      const int r = __shfl(ex ? __builtin_ctz(ex) : 0, L, kWave);
      const float y = stage[r * kWave + L];
      const float s = lse_wave32(coef32 + SB.comp_off, SB, y) -
                      lse_wave32(coef32 + SA.comp_off, SA, y);
      if (lane == L) {
        fold(r, s, y, INFINITY);
        hi_fb = INFINITY;
        if (HOOKS && out_eps) out_eps[J.out_off + t0 + r] = INFINITY;
        ex &= ex - 1;
      }
    }
  }
  // the lane's best lower bound and largest upper bound
  float lo_t = lo_fb, hi_t = hi_fb;
  if (bs_cubic > -INFINITY) {
    const float e = eps_of(bs_cubic);
    lo_t = fmaxf(lo_t, dn(bs_cubic - e));
    hi_t = fmaxf(hi_t, up(bs_cubic + e));
  }
  // one LDS round: the tile's fp32 winner, lo and hi_max (and the fallback
  // count).  np.argmax's order in integers: the wave's largest score order
  // code (NaN canonical: above every number; -0 as +0; 0: no candidate),
  // then the first lane holding it -- lanes are in index order and a lane's
  // own best is its first -- whose key (code, complement of the tile-local
  // index) and y go to LDS; thread 0 forms the block winner's value once.
  const int wid = threadIdx.x / kWave;
  {
    const float a = wave_max_f(lo_t), b = wave_max_f(hi_t);
    uint32_t code = 0u;
    if (br >= 0) code = ord_enc((bs != bs) ? __uint_as_float(0x7FC00000u) : bs + 0.0f);
    uint32_t wc = code;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) wc = max(wc, (uint32_t)__shfl_xor((int)wc, o, kWave));
    const uint64_t own = __ballot(code == wc && wc != 0u);
    if (own != 0ull && lane == (int)__builtin_ctzll(own)) {
      s_key[wid] = ((uint64_t)wc << 32) | (uint64_t)(~(uint32_t)(threadIdx.x * kTRF + br));
      s_wy[wid] = by;
    } else if (own == 0ull && lane == 0) {
      s_key[wid] = 0ull;
    }
    int nf = n_fb;
    if (stats) {
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) nf += __shfl_xor(nf, o, kWave);
    }
    if (lane == 0) {
      s_lo[wid] = a;
      s_hi[wid] = b;
      s_cnt[wid] = nf;
    }
    if (threadIdx.x == 0) s_n = 0;
  }
  __syncthreads();
  float lo_blk = s_lo[0], hi_blk = s_hi[0];
  if (threadIdx.x == 0) {
    uint64_t k = s_key[0];
    int kw = 0, ne = s_cnt[0];
#pragma unroll
    for (int w = 1; w < kBS / kWave; ++w) {
      if (s_key[w] > k) {
        k = s_key[w];
        kw = w;
      }
      ne += s_cnt[w];
    }
    *P = k == 0ull ? empty_best()
                   : tpe_best{(double)ord_dec((uint32_t)(k >> 32)),
                              J.cand_base + base + (int64_t)(~(uint32_t)k),
                              cand_value(s_wy[kw], lgmm), 0};
    if (stats && ne) atomicAdd(stats, (unsigned long long)ne);
  }
#pragma unroll
  for (int w = 1; w < kBS / kWave; ++w) {
    lo_blk = fmaxf(lo_blk, s_lo[w]);
    hi_blk = fmaxf(hi_blk, s_hi[w]);
  }
  if (HOOKS && out_eps) {  // (test hook) the bound of every cubic-scored candidate
#pragma unroll
    for (int r = 0; r < kTRF; ++r)
      if (r < nvalid && !((fbm >> r) & 1u)) {
        const float v = stage[r * kWave + lane];
        out_eps[J.out_off + t0 + r] = (double)up(v + eps_of(v)) - (double)v;
      }
  }
#ifdef TPE_DIAG_NO_BAND  // diagnostic builds only: the fp32 winner alone
  return;
#endif
  // ---- the band tile: its candidates with hi >= lo_blk (NaN hi included);
  // only a lane whose largest upper bound reaches lo_blk holds any.  A
  // cubic-scored candidate's hi = up(s + eps(s)) is monotone in s, so it is
  // tested as s >= s_thr, s_thr = a value below every s with hi >= lo_blk
  // (s + eps(s) < lo_blk whenever s < s_thr: eps(s) <= ea' + 2^-22 |s|, the
  // 2^-20 |lo_blk| slack covers the outward roundings); its hi is formed
  // only for the entries written.  Fallback candidates carry their hi in the
  // stage (two-polynomial) or are always in (log-sum-exp: +inf).
  const float s_thr = lo_blk - fmaf(0x1.0p-20f, fabsf(lo_blk), ea * 1.0001f) - 1e-30f;
  uint32_t em = 0;
  if (!(hi_t < lo_blk)) {
#pragma unroll
    for (int r = 0; r < kTRF; ++r) {
      if (r < nvalid) {
        const float v = stage[r * kWave + lane];
        const bool in = ((fbm >> r) & 1u) ? (((lsem >> r) & 1u) || !(v < lo_blk)) : !(v < s_thr);
        if (in) em |= 1u << r;
      }
    }
  }
  const int cnt = __popc(em);
  const int pos0 = cnt ? atomicAdd(&s_n, cnt) : 0;  // (LDS; the entries' order is free)
  __syncthreads();
  const int total = s_n;
  if (total <= tile_cap && em) {
    tpe_band* B = band + ((int64_t)job * n_tiles + bx) * kTileSlots;
    int pos = pos0;
    // over the lane's entries only (usually one: its own best, whose value
    // it holds; any other entry is drawn again -- exactly as above -- so the
    // draws need not live through the tail)
    for (uint32_t m = em; m; m &= m - 1) {
      const int r = __builtin_ctz(m);
      const float yv = r == br ? by : redraw(J.cand_base + t0 + r);
      const float v = stage[r * kWave + lane];
      const float hi = ((lsem >> r) & 1u) ? INFINITY : ((fbm >> r) & 1u) ? v : up(v + eps_of(v));
      B[pos] = tpe_band{J.cand_base + t0 + r, yv, hi};
      ++pos;
    }
  }
  if (threadIdx.x == 0) {
    hdr[0] = __float_as_uint(lo_blk);
    hdr[1] = __float_as_uint(hi_blk == hi_blk ? hi_blk : INFINITY);
    hdr[2] = total <= tile_cap ? (uint32_t)total : kTileFull;
  }
}
}  // namespace
}  // namespace tpe

using namespace tpe;

extern "C" int64_t tpe_table_partials(const tpe_job* host_jobs, int n_jobs) {
  return tiles_per_job(host_jobs, n_jobs, kTiles * kTile) * n_jobs;
}

extern "C" int tpe_score_table(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                               const tpe_seg* segs, const double* mu, const double* sigma,
                               const double* wcdf, const float* coef32, const tpe_table* tables,
                               const float* cells, const double* cand, double* out_bl,
                               double* out_al, double* out_x, tpe_best* partial,
                               int64_t n_partial, tpe_best* best, uint64_t* stats,
                               void* stream) {
  bool inj = false;
  if (!check_gmm_jobs("tpe_score_table", host_jobs, n_jobs, 65535, kJobTable, &inj))
    return TPE_E_ARG;
  if (n_jobs == 0) return TPE_OK;
  if (!jobs || !segs || !mu || !sigma || !wcdf || !coef32 || !tables || !cells || !partial ||
      !best || (inj && !cand)) {
    set_error("tpe_score_table: null pointer");
    return TPE_E_ARG;
  }
  const int64_t gx = tiles_per_job(host_jobs, n_jobs, kTiles * kTile);
  if (!check_partials("tpe_score_table", n_partial, gx * n_jobs)) return TPE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  // one block per (job, tile) work item, in the kernel's XCD order
  const int64_t blocks = xcd_grid("tpe_score_table", gx, n_jobs);
  if (blocks < 0) return TPE_E_UNSUPPORTED;
#ifndef TPE_DIAG_EXTRA_LDS  // diagnostic builds: dynamic LDS padding to lower occupancy
#define TPE_DIAG_EXTRA_LDS 0
#endif
  dispatch_bool(inj, [&](auto INJ) {
    hipLaunchKernelGGL(k_score_table<decltype(INJ)::value>, dim3((unsigned)blocks), dim3(kBS),
                       decltype(INJ)::value ? 0 : TPE_DIAG_EXTRA_LDS, st, jobs, segs, mu, sigma,
                       wcdf, reinterpret_cast<const float4*>(coef32), tables, cells, cand, out_bl,
                       out_al, out_x, partial, (unsigned long long*)stats, (int)gx, n_jobs);
  });
  launch_reduce(jobs, partial, gx, best, n_jobs, st);
  return check_launch("tpe_score_table");
}

extern "C" int tpe_score_table_fast(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                                    const tpe_seg* segs, const double* mu, const double* sigma,
                                    const double* wcdf, const float* coef32,
                                    const tpe_table* tables, const float* cells, tpe_band* band,
                                    uint32_t* band_ctl, double* out_score, double* out_x,
                                    double* out_eps, tpe_best* partial, int64_t n_partial,
                                    int tile_cap, uint64_t* stats, void* stream) {
  bool inj = false;
  if (!check_gmm_jobs("tpe_score_table_fast", host_jobs, n_jobs, 65535, kJobTable, &inj))
    return TPE_E_ARG;
  if (n_jobs == 0) return TPE_OK;
  if (inj) {
    set_error("tpe_score_table_fast: sampled jobs only (injected candidates: tpe_score_table)");
    return TPE_E_ARG;
  }
  if (!jobs || !segs || !mu || !sigma || !wcdf || !coef32 || !tables || !cells || !band ||
      !band_ctl || !partial) {
    set_error("tpe_score_table_fast: null pointer");
    return TPE_E_ARG;
  }
  if (tile_cap < 0 || tile_cap > kTileSlots) {
    set_error("tpe_score_table_fast: tile_cap=%d (0..%d)", tile_cap, kTileSlots);
    return TPE_E_ARG;
  }
  const int64_t gx = tpe_table_fast_tiles(host_jobs, n_jobs);
  if (!check_partials("tpe_score_table_fast", n_partial, gx * n_jobs)) return TPE_E_ARG;
  const int64_t blocks = xcd_grid("tpe_score_table_fast", gx, n_jobs);
  if (blocks < 0) return TPE_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  dispatch_bool(out_score || out_x || out_eps, [&](auto HOOKS) {
    hipLaunchKernelGGL(k_score_table_fast<decltype(HOOKS)::value>, dim3((unsigned)blocks),
                       dim3(kBS), 0, st, jobs, segs, mu, sigma, wcdf,
                       reinterpret_cast<const float4*>(coef32), tables, cells, band, band_ctl,
                       out_score, out_x, out_eps, partial, (unsigned long long*)stats, (int)gx,
                       n_jobs, tile_cap);
  });
  return check_launch("tpe_score_table_fast");
}
