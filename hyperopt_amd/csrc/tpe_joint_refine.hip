// tpe_joint_refine.hip -- the picked rows climb the joint criterion
// (tpe.suggest_sampled(joint=True, refine=N), tpe.refine_configs; the model:
// hyperopt_amd/joint.py "Refining").
//
// On the continuous labels J(t) = log L_below(t) - log L_above(t) is smooth in
// the fit coordinate t, with per set
//
//   r_i      = exp(a_i - log L)
//   dlogL_d  = sum_i r_i (mu_{i,d} - t_d) / sigma_{i,d}^2
//
// and a row moves by t' = clamp(t + h s^2 g), g = dlogL_below - dlogL_above, s
// the below set's bandwidths: with h = 1 and no above term the mean-shift step
// of the below mixture.  A step is kept when J rises (then h = min(1, 2 h)),
// else h halves; `refine` steps at the most, none once h < 2^-20.
//
// The shape is the reverse of the scorers': a handful of rows against 10^4
// components, refine + 1 evaluations in sequence.  So
//
//   one block per row, the whole climb in one launch;
//   components strided over the block's 256 threads: the prepared set's JComp
//     array is label-major D x C, a wave reads 64 consecutive components of a
//     label;
//   a thread walks its components once per evaluation and keeps an online
//     (m, s, w[D_c]) in registers -- the running maximum of a_i, the sum of
//     exp(a_i - m) and the D_c sums of exp(a_i - m) (mu - t) / sigma^2,
//     rescaled when m rises: value and gradient from one walk;
//   the pairs merge across the wave by a butterfly (four DPP steps inside a
//     row, two shuffles across rows; a merge is commutative bit for bit, so
//     every lane ends with the same bits), then across the four waves through
//     LDS in wave order;
//   LDS holds the row's t (current and trial), g, the moving labels' records
//     and the fixed labels' per-row inputs (a quantized label's clipped edges,
//     a discrete label's hit / miss / prior entries), formed once per row.
//     Their factors differ per component, so they stay in the walk; they are
//     added first, then the moving labels' in list order;
//   the block takes the accept / halve decision: every thread holds the same
//     J and h.
//
// The kernel is instantiated for D_c <= 4, 8 and 16 (the register arrays are
// indexed statically).  No atomics, every sum has a fixed order: a row's bits
// depend on the row, the two sets and `refine` only.
// (The device code lives in tpe_joint_refine.hpp, shared with the tree climb of
// tpe_joint_refine_tree.hip.)
#include "tpe_joint_refine.hpp"

namespace tpe {
namespace {
template <int DC>
__global__ __launch_bounds__(kJBS) void k_joint_refine(const tpe_joint_label* __restrict__ labels,
                                                       int n_labels,
                                                       const double* __restrict__ tables,
                                                       const double* __restrict__ set_b,
                                                       int64_t n_b,
                                                       const double* __restrict__ set_a,
                                                       int64_t n_a, double* __restrict__ vals,
                                                       int64_t ld, int refine,
                                                       double* __restrict__ J_start,
                                                       double* __restrict__ J_end,
                                                       double* __restrict__ g_end,
                                                       int32_t* __restrict__ accepted) {
  __shared__ RShared<DC> sh;
  const int64_t row = blockIdx.x;
  refine_setup<DC>(labels, n_labels, tables, set_b, n_b, set_a, n_a, vals, ld, row, sh);
  const RSet below = refine_set(set_b, n_b, n_labels), above = refine_set(set_a, n_a, n_labels);
  double J0;
  int acc;
  const double J = refine_climb<DC, false>(below, above, nullptr, sh, refine, J0, acc);
  refine_store<DC>(sh, vals, ld, row, g_end ? g_end + row * sh.n_cont : nullptr);
  if (threadIdx.x == 0) {
    if (J_start) J_start[row] = J0;
    if (J_end) J_end[row] = J;
    if (accepted) accepted[row] = acc;
  }
}

template <int DC>
void launch_refine(int64_t n_rows, hipStream_t st, const tpe_joint_label* labels, int n_labels,
                   const double* tables, const double* set_b, int64_t n_b, const double* set_a,
                   int64_t n_a, double* vals, int64_t ld, int refine, double* J_start,
                   double* J_end, double* g_end, int32_t* accepted) {
  hipLaunchKernelGGL(k_joint_refine<DC>, dim3((unsigned)n_rows), dim3(kJBS), 0, st, labels,
                     n_labels, tables, set_b, n_b, set_a, n_a, vals, ld, refine, J_start, J_end,
                     g_end, accepted);
}
}  // namespace
}  // namespace tpe

using namespace tpe;

extern "C" int tpe_joint_refine(const tpe_joint_label* host_labels, const tpe_joint_label* labels,
                                int n_labels, const double* tables, int64_t n_tables,
                                const double* set_below, int64_t n_below, const double* set_above,
                                int64_t n_above, double* vals, int64_t ld, int n_cols,
                                int64_t n_rows, int refine, double* J_start, double* J_end,
                                double* g_end, int32_t* accepted, void* stream) {
  const int rc = check_joint_labels("tpe_joint_refine", host_labels, n_labels, n_cols,
                                    n_tables < 0 ? 0 : n_tables);
  if (rc != TPE_OK) return rc;
  if (n_below < 0 || n_above < 0 || n_below >= ((int64_t)1 << 40) ||
      n_above >= ((int64_t)1 << 40) || n_rows < 0 || ld < 0 || n_rows > ld ||
      n_rows > 2147483647 || refine < 0) {
    set_error("tpe_joint_refine: n=%lld / %lld, n_rows=%lld of ld=%lld, refine=%d",
              (long long)n_below, (long long)n_above, (long long)n_rows, (long long)ld, refine);
    return TPE_E_ARG;
  }
  bool cat = false;
  int n_cont = 0;
  for (int d = 0; d < n_labels; ++d) {
    cat |= host_labels[d].kind == TPE_JOINT_CAT;
    n_cont += host_labels[d].kind == TPE_JOINT_CONT;
  }
  if (n_cont > kRMaxCont) {
    set_error("tpe_joint_refine: %d continuous labels, at most %d", n_cont, kRMaxCont);
    return TPE_E_UNSUPPORTED;
  }
  // (no label moves: nothing to write unless the trace is wanted, and J once)
  if (n_rows == 0 || (n_cont == 0 && !J_start && !J_end && !accepted)) return TPE_OK;
  if (n_cont == 0) refine = 0;
  if (!labels || !set_below || !set_above || !vals || (cat && !tables)) {
    set_error("tpe_joint_refine: null pointer");
    return TPE_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  if (n_cont <= 4)
    launch_refine<4>(n_rows, st, labels, n_labels, tables, set_below, n_below, set_above, n_above,
                     vals, ld, refine, J_start, J_end, g_end, accepted);
  else if (n_cont <= 8)
    launch_refine<8>(n_rows, st, labels, n_labels, tables, set_below, n_below, set_above, n_above,
                     vals, ld, refine, J_start, J_end, g_end, accepted);
  else
    launch_refine<kRMaxCont>(n_rows, st, labels, n_labels, tables, set_below, n_below, set_above,
                             n_above, vals, ld, refine, J_start, J_end, g_end, accepted);
  return check_launch("tpe_joint_refine");
}

extern "C" int tpe_joint_refine_max_cont(void) { return kRMaxCont; }
