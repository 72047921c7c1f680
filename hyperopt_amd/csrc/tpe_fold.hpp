// tpe_fold.hpp -- np.bincount's sequential fp64 sum, parallel and bit-exact.
//
// np.bincount (pyll/base.py:1053-1060) adds the LF weights of a category's
// observations sequentially in observation order, fl(..fl(fl(c + w0) + w1)..),
// and the categorical counts (tpe_fit.hip) must be that chain's bits.  This
// header is the chain's only statement: the pass, the serial prefix and the
// two list drivers (one wave over a list in LDS; one block over a list in
// global memory).  Precondition everywhere: entries finite and >= 0.
//
// The sequential fp64 sum S_{k+1} = fl(S_k + w_k) over list[0, n).  While S
// stays in one binade [2^e, 2^(e+1)) its values are A * u (u = 2^(e-52),
// A < 2^53 an integer) and each step adds d_k * u with d_k = w_k / u rounded
// to an integer -- nearest, ties to the even A_{k+1} (IEEE
// round-to-nearest-even on the binade's grid).  d_k is a shift of w_k's
// mantissa except at a tie (remainder exactly u/2), where it depends on the
// parity of A_k; parities compose as maps P -> a P ^ c (a tie: P -> 0, else
// P -> P ^ (d_k & 1)), so one scan of those maps and one of the d_k give
// every A_k.  The first step whose A would reach 2^53 (the next binade, where
// the grid is 2u), or whose w_k is at least 2^(e+1), is taken by the hardware
// add from its exact predecessor, and the pass repeats from the step after
// it.  Passes: one per list plus one per binade crossed.  (Checked against the
// serial chain on LF ramps, dyadic tie-heavy weights and 24-decade ranges:
// tests/test_seq_fold.py restates it on the host, tests/test_gpu_fold.py runs
// this code on the same lists through tpe_fold_check; the posterior tests
// compare the counts with np.bincount's.)
#pragma once

#include <algorithm>

#include "tpe_common.hpp"

namespace tpe {

// parity maps P -> a P ^ c packed as a | c << 1; y (earlier) then x
__device__ __forceinline__ uint32_t map_then(uint32_t y, uint32_t x) {
  const uint32_t a2 = x & 1u, c2 = (x >> 1) & 1u;
  return (a2 & y & 1u) | ((((a2 & (y >> 1)) ^ c2) & 1u) << 1);
}
template <int CTRL, int ROWM>
__device__ __forceinline__ void scan_step_map(uint32_t& x) {
  x = map_then(dpp_u32<CTRL, ROWM>(1u, x), x);  // (1: the identity map)
}

// The same sum by lane 0 alone (list reads batched; every lane returns it):
// one dependent fp64 add per entry, cheaper than the passes while the sum is
// small and crosses a binade every few entries (the first ~4k of a chain: a
// pass per crossing)
constexpr int kSerialHits = 4096;
static __device__ double serial_fold(double S, const double* list, int n, int lane) {
  if (lane == 0) {
    constexpr int kB = 8;
    int j = 0;
    for (; j + kB <= n; j += kB) {
      double v[kB];
#pragma unroll
      for (int i = 0; i < kB; ++i) v[i] = list[j + i];
#pragma unroll
      for (int i = 0; i < kB; ++i) S = __dadd_rn(S, v[i]);
    }
    for (; j < n; ++j) S = __dadd_rn(S, list[j]);
  }
  return __shfl(S, 0, kWave);
}

// one entry's d (w / u rounded on the binade of biased exponent es, ties
// left for the parity scan: bit j of tie), or bit j of huge (w >= 2^(e+1))
__device__ __forceinline__ uint64_t fold_step(double w, int es, bool on, uint32_t& tie,
                                              uint32_t& huge, int j) {
  if (!on) return 0;
  constexpr uint64_t kFrac = (1ull << 52) - 1;
  const uint64_t wb = (uint64_t)__double_as_longlong(w);
  const int ew = (int)((wb >> 52) & 0x7ff);
  const uint64_t M = (wb & kFrac) | (ew ? (1ull << 52) : 0ull);
  const int sh = es - max(ew, 1);
  if (sh < 0) {
    huge |= 1u << j;
    return 0;
  }
  if (sh == 0) return M;
  if (sh >= 64) return 0;
  const uint64_t rem = M & ((1ull << sh) - 1), half = 1ull << (sh - 1);
  if (rem == half) tie |= 1u << j;
  return (M >> sh) + (rem > half ? 1ull : 0ull);
}

// a block pass's cross-wave exchanges (LDS)
template <int kWaves>
struct FoldX {
  uint32_t wmap[kWaves];   // each wave's composed parity map (inclusive)
  uint64_t wsum[kWaves];   // each wave's increment total
  int64_t wcross[kWaves];  // each wave's first leaving entry (-1: none) ...
  uint64_t wcum[kWaves];   // ... and the increments before it
  double S;                // (the serial prefix's result, broadcast)
};

// The passes over list[0, n), n <= kSE * 64 * kWaves, by kWaves waves (threads
// 0 .. 64 * kWaves - 1, thread t holding entries t * kSE ..; lane: the
// caller's lane_id()); every thread returns the sum.  One wave (kWaves == 1,
// X unused) touches no LDS of its own
// and meets no barrier: k_cat_counts calls it per wave, k_cat_counts_hist from
// wave 0 while the other waves scan.  A block (kWaves > 1) scans the maps and
// the increments per wave and combines the waves' totals through X -- three
// exchanges and four barriers a pass, which covers kWaves times the entries:
// a long chain's ~50k weights take ~15 passes of 4 096 instead of ~100 of 512
// (a pass is a latency-bound chain of dependent steps, not throughput).
template <int kSE, int kWaves>
static __device__ double fold_pass(double S, const double* list, int n, int lane,
                                   FoldX<kWaves>* X) {
  constexpr bool kBlock = kWaves > 1;
  const int wid = kBlock ? threadIdx.x / kWave : 0;
  const int t0 = (wid * kWave + lane) * kSE;  // this thread's first entry
  double v[kSE];
#pragma unroll
  for (int j = 0; j < kSE; ++j) {
    const int i = t0 + j;
    v[j] = i < n ? list[i] : 0.0;
  }
  constexpr uint64_t kFrac = (1ull << 52) - 1, kTop = 1ull << 53;
  int r0 = 0;
  while (r0 < n) {  // (uniform over the wave / the block)
    const uint64_t sb = (uint64_t)__double_as_longlong(S);
    const int es = (int)((sb >> 52) & 0x7ff);
    if (S == 0.0 || es == 0) {  // 0 + w = w; a subnormal sum (never on the LF ramp): one add
      S = __dadd_rn(S, list[r0]);
      ++r0;
      continue;
    }
    const uint64_t A = (sb & kFrac) | (1ull << 52);
    uint64_t d[kSE];
    uint32_t tie = 0, huge = 0;
#pragma unroll
    for (int j = 0; j < kSE; ++j) {
      const int i = t0 + j;
      d[j] = fold_step(v[j], es, i >= r0 && i < n, tie, huge, j);
    }
    // parity maps (bit 0: a, bit 1: c), composed over the lane, then an
    // inclusive wave scan (later o earlier: a = a2 a1, c = a2 c1 ^ c2)
    uint32_t a = 1, c = 0;
#pragma unroll
    for (int j = 0; j < kSE; ++j) {
      if ((tie >> j) & 1u) {
        a = 0;
        c = 0;
      } else {
        c ^= (uint32_t)(d[j] & 1ull);
      }
    }
    uint32_t x = a | (c << 1);
    scan_step_map<0x111, 0xF>(x);
    scan_step_map<0x112, 0xF>(x);
    scan_step_map<0x114, 0xF>(x);
    scan_step_map<0x118, 0xF>(x);
    scan_step_map<0x142, 0xA>(x);
    scan_step_map<0x143, 0xC>(x);
    // the map of everything before this lane: wave_shr:1 (lane 0: the identity) ...
    uint32_t in = dpp_u32<0x138, 0xF>(1u, x);
    if constexpr (kBlock) {
      // ... after the waves before this one, composed in order: lane q < wid
      // holds wave q's map (the others the identity), an ordered scan over
      // kWaves lanes
      if (lane == kWave - 1) X->wmap[wid] = x;
      __syncthreads();
      uint32_t pre = (lane < kWaves && lane < wid) ? X->wmap[lane] : 1u;
#pragma unroll
      for (int o = 1; o < kWaves; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)pre, o, kWave);
        pre = lane >= o ? map_then(y, pre) : pre;
      }
      pre = (uint32_t)__builtin_amdgcn_readlane((int)pre, kWaves - 1);
      in = map_then(pre, in);
    }
    uint32_t P = ((in & 1u) & (uint32_t)(A & 1ull)) ^ (in >> 1);
    uint64_t tot = 0;
#pragma unroll
    for (int j = 0; j < kSE; ++j) {
      if ((tie >> j) & 1u) {
        d[j] += (P + d[j]) & 1ull;  // ties to the even A_{k+1}
        P = 0;
      } else {
        P ^= (uint32_t)(d[j] & 1ull);
      }
      tot += d[j];
    }
    const uint64_t incl = wave_prefix_sum_u64(tot);
    uint64_t cum = incl - tot;  // the increments before this lane's entries
    [[maybe_unused]] uint64_t all = 0;  // (block) the whole pass's increments
    if constexpr (kBlock) {
      // the waves' increment totals: before this wave, and all of them
      if (lane == kWave - 1) X->wsum[wid] = incl;
      __syncthreads();
      const uint64_t wsl = lane < kWaves ? X->wsum[lane] : 0ull;
      uint64_t base = lane < wid ? wsl : 0ull;
      all = wsl;
#pragma unroll
      for (int o = 1; o < kWaves; o <<= 1) {  // (lanes 0..kWaves-1 reduce; lane 0's sums broadcast)
        base += shfl_xor_u64(base, o);
        all += shfl_xor_u64(all, o);
      }
      base = readlane_u64(base, 0);
      all = readlane_u64(all, 0);
      cum = base + incl - tot;
    }
    // the first step leaving the binade: in this lane, then in this wave
    int jc = -1;
#pragma unroll
    for (int j = 0; j < kSE; ++j) {
      if (jc < 0) {
        if (((huge >> j) & 1u) || A + cum + d[j] >= kTop) jc = j;
        else cum += d[j];
      }
    }
    const uint64_t bal = __ballot(jc >= 0);
    // the pass's two ends, D: the increments taken on this binade's grid
    // (A + D < 2^53: exact) -- every entry stays, or entry g leaves by the
    // hardware add and the next pass starts after it
    auto stay = [&](uint64_t D) {
      S = ldexp((double)(A + D), es - 1075);
      r0 = n;
    };
    auto leave = [&](uint64_t D, int g) {
      S = __dadd_rn(ldexp((double)(A + D), es - 1075), list[g]);
      r0 = g + 1;
    };
    if constexpr (!kBlock) {
      if (bal == 0) {
        stay(readlane_u64(incl, kWave - 1));
      } else {
        const int L = __ffsll((unsigned long long)bal) - 1;
        leave(readlane_u64(cum, L), L * kSE + __builtin_amdgcn_readlane(jc, L));
      }
    } else {
      // ... then the first wave leaving
      if (lane == 0) {
        if (bal == 0) {
          X->wcross[wid] = -1;
        } else {
          const int L = __ffsll((unsigned long long)bal) - 1;
          X->wcross[wid] = (int64_t)(wid * kWave + L) * kSE + __builtin_amdgcn_readlane(jc, L);
          X->wcum[wid] = readlane_u64(cum, L);
        }
      }
      __syncthreads();
      const uint64_t cb = __ballot(lane < kWaves && X->wcross[lane < kWaves ? lane : 0] >= 0);
      if (cb == 0) {
        stay(all);
      } else {
        const int qc = __ffsll((unsigned long long)cb) - 1;
        leave(X->wcum[qc], (int)X->wcross[qc]);
      }
      __syncthreads();  // (X is rewritten by the next pass)
    }
  }
  return S;
}

// list[0, n) into S by one wave (every lane returns the sum): the first
// entries of a chain (done < kSerialHits, done: the entries folded before
// this list) serially, the rest in passes of kSE * 64
template <int kSE>
static __device__ double fold_list(double S, const double* list, int n, int64_t& done, int lane) {
  int f = 0;
  if (done < kSerialHits) {
    f = (int)std::min<int64_t>(n, kSerialHits - done);
    S = serial_fold(S, list, f, lane);
  }
  constexpr int kN = kSE * kWave;
  for (; f < n; f += kN) S = fold_pass<kSE, 1>(S, list + f, min(kN, n - f), lane, nullptr);
  done += n;
  return S;
}

// The same by a block of kWaves waves over a list in global memory (every
// thread returns the sum): staged through s_l (kSE * 64 * kWaves doubles of
// LDS) a pass's worth at a time, the serial prefix by wave 0, then the block
// passes.  Call by the whole block (n, done block-uniform).
template <int kSE, int kWaves>
static __device__ double block_fold_list(double S, const double* __restrict__ L, int64_t n,
                                         int64_t done, double* s_l, FoldX<kWaves>& X) {
  constexpr int kB = kWaves * kWave, kN = kSE * kB;
  const int lane = lane_id();
  for (int64_t f0 = 0; f0 < n; f0 += kN) {
    const int m = (int)min((int64_t)kN, n - f0);
    double t[kSE];
#pragma unroll
    for (int u = 0; u < kSE; ++u) {  // (all loads in flight, then the stores)
      const int i = u * kB + (int)threadIdx.x;
      t[u] = i < m ? L[f0 + i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kSE; ++u) {
      const int i = u * kB + (int)threadIdx.x;
      if (i < m) s_l[i] = t[u];
    }
    __syncthreads();
    int f = 0;
    if (done < kSerialHits) {  // the chain's first entries: one thread, one add each
      f = (int)min((int64_t)m, kSerialHits - done);
      if (threadIdx.x < kWave) {
        const double sv = serial_fold(S, s_l, f, lane);
        if (threadIdx.x == 0) X.S = sv;
      }
      __syncthreads();
      S = X.S;
    }
    if (f < m) S = fold_pass<kSE, kWaves>(S, s_l + f, m - f, lane, &X);
    done += m;
    __syncthreads();  // (s_l is restaged next)
  }
  return S;
}

// the block fold's shape (k_cath_fold, tpe_fold_check): 8 waves x 8 entries
// per lane measured fastest
#ifndef TPE_FOLD_WAVES  // diagnostic builds: the block fold's waves and entries per lane
#define TPE_FOLD_WAVES 8
#endif
#ifndef TPE_FOLD_SE
#define TPE_FOLD_SE 8
#endif
constexpr int kFW = TPE_FOLD_WAVES;  // waves of the block fold
constexpr int kFB = kFW * kWave;     // its block (512)
constexpr int kFSE = TPE_FOLD_SE;    // entries per lane per pass
constexpr int kFoldN = kFSE * kFB;   // entries per pass / per staged chunk (4 096)

}  // namespace tpe
