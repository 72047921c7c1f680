// tpe_joint_sample.hip -- rows drawn from a set's joint Parzen mixture
// (tpe.Pool.sample(joint=True); the draw rule: hyperopt_amd/joint.py, DESIGN
// 3.5.5; the mixture: tpe_joint.hip).
//
// Row g = row_base + r is one draw from the prepared set's mixture of C = n + 1
// product kernels: a component i, then every joint label from the component's
// own factor.  Counters are {g lo, g hi, attempt, "JOIN"}:
//
//   component   key keys[D], call (g, 0): word x picks the first i with
//               cdf[i] > x 2^-32 cdf[C - 1] (i == n: the prior).
//   label d     key keys[d], attempts a = 0, 1, ... at (g, a):
//     continuous, quantized   t = mu + sigma normal_f64(y, z, w), (mu, sigma)
//               the component's; a bounded kind accepts lo <= t < hi, and after
//               kMaxAttempts rejections the last t is clamped into [lo, hi) as
//               draw64 clamps; x = exp(t) for a log kind; a quantized label
//               stores rint(x / q) q.
//     discrete  attempt 0 only.  Trial component of category c: word x with
//               x 2^-32 (1 + a) < 1 keeps c, otherwise word y picks from the
//               prior probabilities; the prior component picks with word x
//               (the threshold rule of the categorical sampler: first k with
//               word < ceil(cdf[k] / cdf[K - 1] 2^32), the word 2^32 - 1 read
//               as 2^32 - 2).
//
// One thread per (row, label) on a grid of row blocks x labels: the label's
// record is block-uniform, the rejection loop the only divergence, and a
// label's column is written by consecutive threads.  Every thread repeats its
// row's component pick (one Philox call and a search).  A row's values depend
// on (keys, g, the set, the labels) alone: no thread reads another's result,
// there are no atomics, and the row window only moves the row to another
// thread.
#include "tpe_joint.hpp"

namespace tpe {
namespace {
constexpr int kJSBS = 256;                           // threads (rows) per block
constexpr int kJSStage = TPE_JOINT_SAMPLE_STAGE;     // cdf entries staged in LDS
constexpr uint32_t kJSMaxAttempts = 256;             // draw64's kMaxAttempts
constexpr uint32_t kStreamJoint = 0x4A4F494Eu;       // "JOIN"

// first k with cdf[k] > u, the last one if none
__device__ __forceinline__ int64_t first_above(const double* cdf, int64_t n, double u) {
  int64_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (cdf[mid] > u) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// category of `word` under the K-entry cdf: thr[k] = ceil(cdf[k] / cdf[K - 1]
// 2^32) saturated at 2^32 - 1; the first k with word < thr[k], the last if none
__device__ __forceinline__ int category_of_word(const double* __restrict__ cdf, int K,
                                                uint32_t word) {
  const double total = cdf[K - 1];
  word = word < 0xFFFFFFFEu ? word : 0xFFFFFFFEu;
  int lo = 0, hi = K - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const double t = ceil(cdf[mid] / total * 4294967296.0);
    const uint32_t thr = t >= 4294967295.0 ? 0xFFFFFFFFu : (t > 0.0 ? (uint32_t)t : 0u);
    if (word < thr) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// block (row tile, label d): thread r draws label d of row row_base + r
__global__ __launch_bounds__(kJSBS) void k_joint_sample(
    const tpe_joint_label* __restrict__ labels, int n_labels, const double* __restrict__ set,
    int64_t n, const double* __restrict__ cdf, const double* __restrict__ cat_cdf,
    const uint64_t* __restrict__ keys, double one_plus_a, int64_t row_base, int64_t n_rows,
    double* __restrict__ vals, int64_t ld, int32_t* __restrict__ comp_out) {
  __shared__ double s_cdf[kJSStage];
  const int64_t C = n + 1;
  const bool staged = C <= kJSStage;  // (block-uniform)
  if (staged) {
    for (int k = threadIdx.x; k < (int)C; k += kJSBS) s_cdf[k] = cdf[k];
    __syncthreads();
  }
  const int64_t r = (int64_t)blockIdx.x * kJSBS + threadIdx.x;
  if (r >= n_rows) return;
  const int d = blockIdx.y;
  const int64_t g = row_base + r;
  const tpe_joint_label lab = labels[d];

  // the row's component
  const U4 pick = draw_words(keys[n_labels], g, 0u, kStreamJoint);
  int64_t i;
  if (staged) {
    i = first_above(s_cdf, C, (double)pick.x * 0x1.0p-32 * s_cdf[C - 1]);
  } else {
    i = first_above(cdf, C, (double)pick.x * 0x1.0p-32 * cdf[C - 1]);
  }
  const bool prior = i == n;
  if (comp_out && d == 0) comp_out[r] = (int32_t)i;

  const uint64_t key = keys[d];
  const JComp* __restrict__ comp = reinterpret_cast<const JComp*>(set + set_comp_off(n_labels, C));
  double v;
  if (lab.kind == TPE_JOINT_CAT) {
    const double* __restrict__ cc = cat_cdf + lab.tab_off / 3;
    const U4 w = draw_words(key, g, 0u, kStreamJoint);
    if (prior) {
      v = (double)category_of_word(cc, lab.n_cat, w.x);
    } else if ((double)w.x * 0x1.0p-32 * one_plus_a < 1.0) {
      v = comp[(int64_t)d * C + i].mu;  // the component's own category
    } else {
      v = (double)category_of_word(cc, lab.n_cat, w.y);
    }
  } else {
    const double mu = prior ? lab.prior_mu : comp[(int64_t)d * C + i].mu;
    const double sigma = prior ? lab.prior_sigma : set[C + d];
    const bool bounded = (lab.flags & TPE_JOINT_BOUNDED) != 0;
    double t = 0.0;
    bool accepted = false;
    for (uint32_t a = 0; a < kJSMaxAttempts; ++a) {
      const U4 w = draw_words(key, g, a, kStreamJoint);
      t = mu + sigma * normal_f64(w.y, w.z, w.w);
      if (!bounded || (lab.lo <= t && t < lab.hi)) {
        accepted = true;
        break;
      }
    }
    if (!accepted) {  // keep the last draw, clamped into the support (draw64)
      if (t < lab.lo) t = lab.lo;
      if (!(t < lab.hi)) t = nextafter(lab.hi, -INFINITY);
    }
    v = (lab.flags & TPE_JOINT_LOG) ? exp(t) : t;
    if (lab.kind == TPE_JOINT_QUANT) v = rint(v / lab.q) * lab.q;
  }
  vals[(int64_t)lab.col * ld + r] = v;
}
}  // namespace
}  // namespace tpe

using namespace tpe;

extern "C" int tpe_joint_sample_stage(void) { return kJSStage; }

extern "C" int tpe_joint_sample(const tpe_joint_label* host_labels, const tpe_joint_label* labels,
                                int n_labels, const double* set, int64_t n, const double* cdf,
                                const double* cat_cdf, int64_t n_cat_cdf, const uint64_t* keys,
                                double one_plus_a, int64_t row_base, int64_t n_rows, double* vals,
                                int64_t ld, int n_cols, int32_t* comp_out, void* stream) {
  const int rc = check_joint_labels("tpe_joint_sample", host_labels, n_labels, n_cols, -1);
  if (rc != TPE_OK) return rc;
  bool cat = false;
  for (int d = 0; d < n_labels; ++d) {
    const tpe_joint_label& l = host_labels[d];
    if (l.kind != TPE_JOINT_CAT) continue;
    cat = true;
    if (l.tab_off % 3 != 0 || n_cat_cdf < 0 || l.tab_off / 3 + (int64_t)l.n_cat > n_cat_cdf) {
      set_error("tpe_joint_sample: label %d: tab_off=%lld (a multiple of 3), its cdf ends at "
                "%lld of %lld", d, (long long)l.tab_off,
                (long long)(l.tab_off / 3 + (int64_t)l.n_cat), (long long)n_cat_cdf);
      return TPE_E_ARG;
    }
  }
  // (a component index is an int32 in comp_out)
  if (n < 0 || n >= 2147483647 || row_base < 0 || n_rows < 0 || ld < 0 || n_rows > ld ||
      row_base > INT64_MAX - n_rows || !(one_plus_a >= 1.0) || !(one_plus_a < INFINITY)) {
    set_error("tpe_joint_sample: n=%lld rows [%lld, +%lld) of ld=%lld, 1 + a = %g", (long long)n,
              (long long)row_base, (long long)n_rows, (long long)ld, one_plus_a);
    return TPE_E_ARG;
  }
  if (n_rows == 0) return TPE_OK;
  if (!labels || !set || !cdf || !keys || !vals || (cat && !cat_cdf)) {
    set_error("tpe_joint_sample: null pointer");
    return TPE_E_ARG;
  }
  const int64_t blocks = (n_rows + kJSBS - 1) / kJSBS;
  if (blocks > 2147483647) {
    set_error("tpe_joint_sample: n_rows=%lld does not fit a launch", (long long)n_rows);
    return TPE_E_ARG;
  }
  hipLaunchKernelGGL(k_joint_sample, dim3((unsigned)blocks, (unsigned)n_labels), dim3(kJSBS), 0,
                     (hipStream_t)stream, labels, n_labels, set, n, cdf, cat_cdf, keys, one_plus_a,
                     row_base, n_rows, vals, ld, comp_out);
  return check_launch("tpe_joint_sample");
}
