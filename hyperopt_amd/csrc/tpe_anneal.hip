// tpe_anneal.hip -- anneal.suggest on the HBM-resident history.
//
// Replaces the per-suggest work of AnnealingAlgo (hyperopt/anneal.py:100-391):
// the walk over every document (miscs_to_idxs_vals), the per-label loss lists
// and their argsort (choose_ltv), and the concentrated draws (hp_uniform ..
// hp_qnormal).  One block per new trial visits the trial's live labels of one
// level in order -- the chain of chosen rows (best_tids) is sequential within
// a trial.  Per label: reuse the first chained row that has the label, or draw
// g = geometric(1 / avg_best_idx) - 1 and take the row of rank g among the
// column's active rows in np.argsort(loss, kind="stable") order.
//
// Selection: a most-significant-digit radix select over order_key(loss) (a
// monotone 64-bit key: -0.0 == +0.0, NaN last), 8 bits per pass, the digit
// histogram in LDS; a pass narrows the candidates to one digit bin, and the
// passes stop as soon as that bin holds one row.  A last pass in ascending row
// order (64-bit __ballot + popcount prefix) takes the k-th row with the
// selected key: ties go to the earlier row.  O(n_rows) per pass, no sort.
//
// Draws: Philox4x32-10 keyed by (label key, new_id), counter word 0 for the
// pick and 1 for the value, so a reused pick does not shift the value's words.
// The formulas follow the reference's operation order (-ffp-contract=off).
#include "tpe_common.hpp"

namespace tpe {
namespace {
constexpr int kABS = 256;
constexpr int kAWaves = kABS / kWave;
constexpr int kDigitBits = 8;
constexpr int kBins = 1 << kDigitBits;  // == kABS: thread d owns bin d
static_assert(kBins == kABS, "one histogram bin per thread");
constexpr uint32_t kStreamAnneal = 0x414E4E4Cu;  // "ANNL"
constexpr uint32_t kCtrPick = 0u, kCtrValue = 1u;

struct SelShared {
  uint32_t hist[kBins];
  uint32_t wsum[kAWaves];
  int32_t digit, rank, count, row, first;
};

// Row of rank k (0-based, clipped to the rows found) among the rows r with
// A[r] != 0 in (order_key(loss[r]), r) order; -1 when there is none.  Every
// thread of the block calls it with the same arguments and gets the same
// result.  *n_found: the number of active rows counted.
__device__ int32_t select_row(const double* __restrict__ loss, const uint8_t* __restrict__ A,
                              int32_t n_rows, int32_t k, SelShared& S, int32_t* n_found) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
  uint64_t prefix = 0, mask = 0;
  for (int pass = 0; pass < 64 / kDigitBits; ++pass) {
    const int shift = 64 - kDigitBits * (pass + 1);
    S.hist[tid] = 0;
    __syncthreads();
    for (int32_t r = tid; r < n_rows; r += kABS) {
      if (!A[r]) continue;
      const uint64_t key = order_key(loss[r]);
      if ((key & mask) == prefix) atomicAdd(&S.hist[(key >> shift) & (kBins - 1)], 1u);
    }
    __syncthreads();
    // inclusive scan of the 256 bins: 64-lane shuffles, then the wave totals
    const uint32_t c = S.hist[tid];
    uint32_t incl = c;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const uint32_t o = __shfl_up(incl, off, kWave);
      if (lane >= off) incl += o;
    }
    if (lane == kWave - 1) S.wsum[wid] = incl;
    __syncthreads();
    uint32_t base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kAWaves; ++w) {
      if (w < wid) base += S.wsum[w];
      total += S.wsum[w];
    }
    incl += base;
    if (pass == 0) {
      *n_found = (int32_t)total;
      if (total == 0) return -1;
      if ((uint32_t)k >= total) k = (int32_t)total - 1;
    }
    const uint32_t excl = incl - c;
    if (c > 0 && excl <= (uint32_t)k && (uint32_t)k < incl) {
      S.digit = tid;
      S.rank = k - (int32_t)excl;
      S.count = (int32_t)c;
    }
    __syncthreads();
    k = S.rank;
    prefix |= (uint64_t)S.digit << shift;
    mask |= (uint64_t)(kBins - 1) << shift;
    if (S.count == 1) break;  // one candidate left: the row pass finds it
  }
  // the k-th row, in ascending row order, among the candidates (all of one key
  // when the eight passes ran; a single row otherwise)
  if (tid == 0) S.row = -1;
  __syncthreads();
  int32_t seen = 0;
  for (int32_t r0 = 0; r0 < n_rows; r0 += kABS) {
    const int32_t r = r0 + tid;
    const bool m = r < n_rows && A[r] && (order_key(loss[r]) & mask) == prefix;
    const unsigned long long bal = __ballot(m);
    if (lane == 0) S.wsum[wid] = (uint32_t)__popcll(bal);
    __syncthreads();
    int32_t before = seen, total = 0;
#pragma unroll
    for (int w = 0; w < kAWaves; ++w) {
      if (w < wid) before += (int32_t)S.wsum[w];
      total += (int32_t)S.wsum[w];
    }
    before += __popcll(bal & ((1ull << lane) - 1ull));
    if (m && before == k) S.row = r;
    seen += total;
    __syncthreads();
    if (seen > k) break;
  }
  return S.row;
}

// first k with cumsum(p)[k] > u * sum(p), p[k] = keep * (k == hot) + mix * prior[k]
// (prior == nullptr: the constant `flat`), walked without storing p
__device__ __forceinline__ int walk_categorical(int K, int hot, double keep, double mix,
                                                const double* __restrict__ prior, double flat,
                                                double u) {
  double tot = 0.0;
  for (int k = 0; k < K; ++k)
    tot += keep * (k == hot ? 1.0 : 0.0) + mix * (prior ? prior[k] : flat);
  const double t = u * tot;
  double c = 0.0;
  int k = 0;
  for (; k < K - 1; ++k) {
    c += keep * (k == hot ? 1.0 : 0.0) + mix * (prior ? prior[k] : flat);
    if (c > t) break;
  }
  return k;
}

__global__ __launch_bounds__(kABS) void k_anneal_sample(
    const double* __restrict__ vals, const uint8_t* __restrict__ active, int64_t ld,
    int32_t n_rows, const double* __restrict__ loss, const tpe_anneal* __restrict__ recs,
    int n_recs, const double* __restrict__ p, const int32_t* __restrict__ item_off,
    const int32_t* __restrict__ item_label, int64_t n_items, const int64_t* __restrict__ new_ids,
    double avg_best_idx, int32_t* chain, int32_t* chain_n, int chain_ld,
    double* __restrict__ out, tpe_anneal_dbg* __restrict__ dbg, int32_t* err) {
  __shared__ SelShared S;
  const int tid = threadIdx.x;
  const int64_t t = blockIdx.x;
  const int64_t lo = item_off[t], hi = item_off[t + 1];
  int32_t n_chain = chain_n[t];
  if (lo < 0 || hi < lo || hi > n_items || n_chain < 0 || n_chain > chain_ld) {
    if (tid == 0) atomicOr(err, 8);
    return;
  }
  int32_t* ch = chain + t * chain_ld;
  const int64_t new_id = new_ids[t];
  const double nan = __longlong_as_double(0x7FF8000000000000ll);

  for (int64_t it = lo; it < hi; ++it) {
    const int lab = item_label[it];
    if (lab < 0 || lab >= n_recs) {
      if (tid == 0) {
        atomicOr(err, 8);
        out[it] = nan;
      }
      continue;
    }
    const tpe_anneal R = recs[lab];
    const uint8_t* A = active + (int64_t)R.col * ld;
    int32_t row = -1, reused = 0, g = -1;
    if (R.n_active > 0) {
      // the first chained row that has this label
      __syncthreads();
      if (tid == 0) S.first = INT32_MAX;
      __syncthreads();
      for (int32_t i = tid; i < n_chain; i += kABS) {
        const int32_t r = ch[i];
        if (r >= 0 && r < n_rows && A[r]) atomicMin(&S.first, i);
      }
      __syncthreads();
      const int32_t first = S.first;
      if (first != INT32_MAX) {
        row = ch[first];
        reused = 1;
      } else {
        // g = geometric(p) - 1 by inversion, clipped in fp64
        const U4 w = draw_words(R.key, new_id, kCtrPick, kStreamAnneal);
        const double pg = 1.0 / avg_best_idx;
        double gd = 0.0;
        if (pg < 1.0) {
          const double u1 = 1.0 - u01_f64(w.x, w.y);  // (0, 1]
          gd = ceil(log(u1) / log1p(-pg)) - 1.0;
          if (!(gd >= 0.0)) gd = 0.0;
        }
        gd = fmin(gd, (double)(R.n_active - 1));
        int32_t n_found = 0;
        row = select_row(loss, A, n_rows, (int32_t)gd, S, &n_found);
        g = (int32_t)gd < n_found ? (int32_t)gd : n_found - 1;
        if (n_found != R.n_active && tid == 0) atomicOr(err, 4);
        if (row >= 0) {
          if (n_chain < chain_ld) {
            if (tid == 0) ch[n_chain] = row;
            ++n_chain;
          } else if (tid == 0) {
            atomicOr(err, 8);
          }
        }
      }
    }
    if (tid != 0) continue;

    // ---- the value: the prior concentrated around the chosen row's value ----
    const U4 w = draw_words(R.key, new_id, kCtrValue, kStreamAnneal);
    const double u = u01_f64(w.x, w.y);  // [0, 1), 53 bits
    const bool prior = row < 0;
    const double val = prior ? 0.0 : vals[(int64_t)R.col * ld + row];
    double v, p0 = R.a, p1 = R.b, variate = u;
    switch (R.kind) {
      case TPE_PRIOR_UNIFORM:
      case TPE_PRIOR_LOGUNIFORM: {
        double low = R.a, high = R.b;
        if (!prior) {
          double mid = R.kind == TPE_PRIOR_LOGUNIFORM ? log(val) : val;
          const double half = 0.5 * ((R.b - R.a) * R.shrink);
          const double mn = R.a + half, mx = R.b - half;
          mid = mid < mn ? mn : mid;  // np.clip (NaN stays NaN)
          mid = mid > mx ? mx : mid;
          low = mid - half;
          high = mid + half;
          p0 = mid;
          p1 = half;
        }
        v = low + (high - low) * u;
        if (R.kind == TPE_PRIOR_LOGUNIFORM) v = exp(v);
        break;
      }
      case TPE_PRIOR_NORMAL:
      case TPE_PRIOR_LOGNORMAL: {
        double mu = R.a, sigma = R.b;
        if (!prior) {
          mu = val;
          if (R.kind == TPE_PRIOR_LOGNORMAL) mu = log(R.q > 0.0 ? 1e-16 + val : val);
          sigma = R.b * R.shrink;
          p0 = mu;
          p1 = sigma;
        }
        variate = normal_f64(w.x, w.y, w.z);
        v = mu + sigma * variate;
        if (R.kind == TPE_PRIOR_LOGNORMAL) v = exp(v);
        break;
      }
      case TPE_PRIOR_RANDINT: {
        const double K = R.b - R.a;
        if (prior) {
          v = R.a + fmin(floor(u * K), K - 1.0);
        } else {
          const int hot = (int)(val - R.a);
          v = R.a + (double)walk_categorical((int)K, hot, 1.0 - R.shrink, R.shrink, nullptr,
                                             1.0 / K, u);
          p0 = (double)hot;
          p1 = R.shrink;
        }
        break;
      }
      default: {  // categorical
        const int hot = prior ? -1 : (int)val;
        const double mix = prior ? 1.0 : R.shrink;
        v = (double)walk_categorical(R.n_cat, hot, 1.0 - mix, mix, p + R.p_off, 0.0, u);
        if (!prior) {
          p0 = (double)hot;
          p1 = R.shrink;
        }
      }
    }
    if (R.q > 0.0) v = rint(v / R.q) * R.q;
    out[it] = v;
    if (dbg) dbg[it] = tpe_anneal_dbg{row, reused, g, 0, p0, p1, variate};
  }
  if (tid == 0) chain_n[t] = n_chain;
}
}  // namespace
}  // namespace tpe

using namespace tpe;

extern "C" int tpe_anneal_struct_sizes(int32_t* out, int n) {
  const int32_t s[2] = {(int32_t)sizeof(tpe_anneal), (int32_t)sizeof(tpe_anneal_dbg)};
  for (int i = 0; i < n && i < 2; ++i) out[i] = s[i];
  return 2;
}

extern "C" int tpe_anneal_sample(const double* vals, const uint8_t* active, int64_t ld,
                                 int64_t n_cols, int64_t n_rows, const double* loss,
                                 const tpe_anneal* recs, const tpe_anneal* host_recs, int n_recs,
                                 const double* p, const int32_t* item_off,
                                 const int32_t* item_label, int64_t n_items,
                                 const int64_t* new_ids, int64_t n_trials, double avg_best_idx,
                                 int32_t* chain, int32_t* chain_n, int chain_ld, double* out,
                                 tpe_anneal_dbg* dbg, int32_t* err, void* stream) {
  if (n_recs < 0 || n_trials < 0 || n_items < 0 || n_rows < 0 || n_cols < 0 || ld < n_rows ||
      chain_ld < 0 || (n_recs > 0 && !host_recs)) {
    set_error("tpe_anneal_sample: bad arguments (n_recs=%d n_trials=%lld n_items=%lld "
              "n_rows=%lld ld=%lld)", n_recs, (long long)n_trials, (long long)n_items,
              (long long)n_rows, (long long)ld);
    return TPE_E_ARG;
  }
  if (!(avg_best_idx > 0.0)) {
    set_error("tpe_anneal_sample: avg_best_idx must be positive");
    return TPE_E_ARG;
  }
  if (n_trials == 0 || n_items == 0) return TPE_OK;
  if (n_rows > INT32_MAX || n_items > INT32_MAX) {
    set_error("tpe_anneal_sample: n_rows=%lld / n_items=%lld too large", (long long)n_rows,
              (long long)n_items);
    return TPE_E_UNSUPPORTED;
  }
  for (int j = 0; j < n_recs; ++j) {
    const tpe_anneal& R = host_recs[j];
    if (R.kind < TPE_PRIOR_UNIFORM || R.kind > TPE_PRIOR_CATEGORICAL) {
      set_error("tpe_anneal_sample: record %d has kind %d", j, R.kind);
      return TPE_E_ARG;
    }
    if (R.kind == TPE_PRIOR_CATEGORICAL && (R.n_cat < 1 || R.p_off < 0 || !p)) {
      set_error("tpe_anneal_sample: categorical record %d without probabilities", j);
      return TPE_E_ARG;
    }
    if (R.kind == TPE_PRIOR_RANDINT && !(R.b > R.a)) {
      set_error("tpe_anneal_sample: randint record %d has high <= low", j);
      return TPE_E_ARG;
    }
    if (R.kind == TPE_PRIOR_RANDINT && R.b - R.a > (double)INT32_MAX) {
      set_error("tpe_anneal_sample: randint record %d has too many values", j);
      return TPE_E_UNSUPPORTED;
    }
    if (R.col < 0 || R.col >= n_cols || R.n_active < 0 || R.n_active > n_rows) {
      set_error("tpe_anneal_sample: record %d has column %d (of %lld), n_active %d (of %lld rows)",
                j, R.col, (long long)n_cols, R.n_active, (long long)n_rows);
      return TPE_E_ARG;
    }
  }
  if (chain_ld < n_recs) {
    set_error("tpe_anneal_sample: chain_ld=%d below the %d labels", chain_ld, n_recs);
    return TPE_E_ARG;
  }
  if (!vals || !active || !loss || !recs || !item_off || !item_label || !new_ids || !chain ||
      !chain_n || !out || !err) {
    set_error("tpe_anneal_sample: null pointer");
    return TPE_E_ARG;
  }
  if (n_trials > INT32_MAX) {
    set_error("tpe_anneal_sample: n_trials=%lld too large", (long long)n_trials);
    return TPE_E_UNSUPPORTED;
  }
  hipLaunchKernelGGL(k_anneal_sample, dim3((unsigned)n_trials), dim3(kABS), 0,
                     (hipStream_t)stream, vals, active, ld, (int32_t)n_rows, loss, recs, n_recs, p,
                     item_off, item_label, n_items, new_ids, avg_best_idx, chain, chain_n,
                     chain_ld, out, dbg, err);
  return check_launch("tpe_anneal_sample");
}
