// tpe_joint_refine_tree.hip -- the picked rows climb their groups under
// joint="tree" (tpe.suggest_sampled(joint="tree", refine_tree=N),
// tpe.refine_configs(joint="tree"); the model: hyperopt_amd/joint.py "Refining in
// a tree").
//
// S(c) = sum_g J_g(c_g) over disjoint label groups, so the climb of
// tpe_joint_refine.hip separates exactly: one independent climb per (row, group
// live in the row), with the group's sets, gradient, bandwidths, h and stop.  The
// arithmetic is tpe_joint_refine.hpp's, shared with the flat kernel; what is new
// is the shape of the work and where a walk reads from.
//
//   grid     blockIdx.x the row, blockIdx.y a group of one instantiation class
//            (D_c <= 4 / 8 / 16; the class's group indices travel in the kernel
//            arguments): at most three launches.  A block reads its group's
//            record from the device copy of the group table -- the index is
//            block-uniform, so the record arrives by scalar loads -- and, where
//            the group is not live in the row, writes the pair's NaN / 0 outputs
//            and returns before it touches LDS or `vals`.
//   staging  a climb evaluates the same two sets refine + 1 times, and a group's
//            sets are small: a below set never exceeds 26 components, a branch's
//            above set holds the trials that took the branch.  At block start
//            the 256 threads copy a set into LDS -- log w, then the group's
//            JComp rows, which are contiguous in the prepared buffer (label-
//            major D x C), as 16-byte loads and stores, a wave 1 KB at a time --
//            and every evaluation walks the copy.  The stage is one static
//            array: the below set's place is sized for its 26 components, the
//            above set stages when it fits the rest (stage_components), and a
//            set that does not is streamed from L2 as the flat kernel streams
//            it.  Thread i owns components i, i + 256, ... either way.
//   LDS      RShared<DC> (<= 8.8 KB) + the 54 KB stage: static, under 64 KB per
//            block, two blocks per CU.
//
// No atomics, every sum in a fixed order: a pair's bits depend on the row, the
// group's two sets and `refine` alone, and are the flat kernel's on the same
// inputs, staged or streamed.
#include "tpe_joint_refine.hpp"

namespace tpe {
namespace {
constexpr int kRBelowMax = 26;  // components of a below set: split_masks keeps <= 25 trials
constexpr int kRStageDoubles = 54 * 1024 / 8;

// a staged set's doubles: log w padded to an even count, D x C pairs
__host__ __device__ constexpr int64_t stage_doubles(int64_t C, int D) {
  return stage_comp_off(C) + 2 * (int64_t)D * C;
}

static_assert(sizeof(RShared<kRMaxCont>) + 8 * kRStageDoubles <= 64 * 1024,
              "static LDS stays within 64 KB per block");
static_assert(stage_doubles(kRBelowMax, kJMaxD) <= kRStageDoubles,
              "a below set of the widest group stages");
static_assert(stage_doubles(kRBelowMax, 1) % 2 == 0, "the above set's copy is 16-byte aligned");

// the largest C at which a D-label group's above set stages behind its below set's place
__host__ __device__ inline int64_t stage_components(int D) {
  const int64_t rest = kRStageDoubles - stage_doubles(kRBelowMax, D);
  int64_t C = rest / (2 * (int64_t)D + 1);
  while (C > 0 && stage_doubles(C, D) > rest) --C;
  return C;
}

// the groups of one launch: blockIdx.y -> group
struct RClass {
  int n;
  int32_t g[kJMaxD];
};

// the block's copy of a set of C components of D labels into dst (16-byte
// aligned, as the set is); the caller syncs
__device__ __forceinline__ void refine_stage(double* dst, const RSet& set, int D) {
  const int64_t C = set.n + 1;
  for (int64_t i = threadIdx.x; i < C; i += kJBS) dst[i] = set.logw[i];
  const double2* __restrict__ src = reinterpret_cast<const double2*>(set.comp);
  double2* out = reinterpret_cast<double2*>(dst + stage_comp_off(C));
  for (int64_t e = threadIdx.x; e < (int64_t)D * C; e += kJBS) out[e] = src[e];
}

template <int DC>
__global__ __launch_bounds__(kJBS) void k_joint_refine_tree(
    const tpe_joint_label* __restrict__ labels, const double* __restrict__ tables,
    const tpe_refine_group* __restrict__ groups, const RClass cls, int n_groups, int dc_tot,
    double* vals, const uint8_t* __restrict__ active, int64_t ld, int refine,
    double* __restrict__ J_start, double* __restrict__ J_end, double* __restrict__ g_end,
    int32_t* __restrict__ accepted) {
  __shared__ RShared<DC> sh;
  __shared__ __attribute__((aligned(16))) double stage[kRStageDoubles];
  const int g = cls.g[blockIdx.y];
  const tpe_refine_group grp = groups[g];
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t at = row * n_groups + g;
  double* g_row = g_end ? g_end + row * dc_tot + grp.g_off : nullptr;
  if (grp.live_col >= 0 && active[(int64_t)grp.live_col * ld + row] == 0) {
    if (tid == 0) {
      if (J_start) J_start[at] = NAN;
      if (J_end) J_end[at] = NAN;
      if (accepted) accepted[at] = 0;
    }
    if (g_row && tid < grp.n_cont) g_row[tid] = NAN;
    return;
  }
  const int D = grp.count;
  refine_setup<DC>(labels + grp.first, D, tables ? tables + grp.tab_off : nullptr, grp.set_below,
                   grp.n_below, grp.set_above, grp.n_above, vals, ld, row, sh);
  RSet below = refine_set(grp.set_below, grp.n_below, D);
  RSet above = refine_set(grp.set_above, grp.n_above, D);
  if (grp.n_below + 1 <= kRBelowMax) {
    below.stage_off = 0;
    refine_stage(stage, below, D);
  }
  if (grp.n_above + 1 <= stage_components(D)) {
    above.stage_off = (int)stage_doubles(kRBelowMax, D);
    refine_stage(stage + above.stage_off, above, D);
  }
  __syncthreads();
  double J0;
  int acc;
  // (a group without a moving label: J once, as tpe_joint_refine has it)
  const double J =
      refine_climb<DC, true>(below, above, stage, sh, sh.n_cont ? refine : 0, J0, acc);
  refine_store<DC>(sh, vals, ld, row, g_row);
  if (tid == 0) {
    if (J_start) J_start[at] = J0;
    if (J_end) J_end[at] = J;
    if (accepted) accepted[at] = acc;
  }
}

template <int DC>
void launch_refine_tree(const RClass& cls, int64_t n_rows, hipStream_t st,
                        const tpe_joint_label* labels, const double* tables,
                        const tpe_refine_group* groups, int n_groups, int dc_tot, double* vals,
                        const uint8_t* active, int64_t ld, int refine, double* J_start,
                        double* J_end, double* g_end, int32_t* accepted) {
  if (cls.n == 0) return;
  hipLaunchKernelGGL(k_joint_refine_tree<DC>, dim3((unsigned)n_rows, (unsigned)cls.n), dim3(kJBS),
                     0, st, labels, tables, groups, cls, n_groups, dc_tot, vals, active, ld,
                     refine, J_start, J_end, g_end, accepted);
}
}  // namespace
}  // namespace tpe

using namespace tpe;

extern "C" int tpe_joint_refine_tree(const tpe_joint_label* host_labels,
                                     const tpe_joint_label* labels, int n_labels,
                                     const double* tables, int64_t n_tables,
                                     const tpe_refine_group* host_groups,
                                     const tpe_refine_group* groups, int n_groups, double* vals,
                                     const uint8_t* active, int64_t ld, int n_cols,
                                     int64_t n_rows, int refine, double* J_start, double* J_end,
                                     double* g_end, int32_t* accepted, void* stream) {
  const char* fn = "tpe_joint_refine_tree";
  if (n_groups < 1 || n_labels < 1 || !host_groups || !host_labels) {
    set_error("%s: n_groups=%d, n_labels=%d / null host arrays", fn, n_groups, n_labels);
    return TPE_E_ARG;
  }
  if (n_groups > kJMaxD || n_labels > kJMaxD) {
    set_error("%s: %d groups of %d labels in all, at most %d of either", fn, n_groups, n_labels,
              kJMaxD);
    return TPE_E_UNSUPPORTED;
  }
  if (n_rows < 0 || ld < 0 || n_rows > ld || n_rows > 2147483647 || refine < 0 || n_tables < 0) {
    set_error("%s: n_rows=%lld of ld=%lld, refine=%d, n_tables=%lld", fn, (long long)n_rows,
              (long long)ld, refine, (long long)n_tables);
    return TPE_E_ARG;
  }
  const bool want_J = J_start || J_end || accepted;
  RClass cls[3];
  cls[0].n = cls[1].n = cls[2].n = 0;
  int dc_tot = 0;
  bool cat = false, cond = false;
  for (int g = 0; g < n_groups; ++g) {
    const tpe_refine_group& r = host_groups[g];
    if (r.first < 0 || r.count < 1 || r.first > n_labels - r.count || r.live_col < -1 ||
        r.live_col >= n_cols || r.tab_off < 0 || r.tab_off > n_tables || r.n_below < 0 ||
        r.n_above < 0 || r.n_below >= ((int64_t)1 << 40) || r.n_above >= ((int64_t)1 << 40) ||
        !r.set_below || !r.set_above || ((uintptr_t)r.set_below & 15) ||
        ((uintptr_t)r.set_above & 15)) {
      set_error("%s: group %d: labels [%d, +%d) of %d, column %d of %d, tab_off=%lld, n=%lld / "
                "%lld, or a set that is null or not 16-byte aligned", fn, g, r.first, r.count,
                n_labels, r.live_col, n_cols, (long long)r.tab_off, (long long)r.n_below,
                (long long)r.n_above);
      return TPE_E_ARG;
    }
    const int rc = check_joint_labels(fn, host_labels + r.first, r.count, n_cols,
                                      n_tables - r.tab_off);
    if (rc != TPE_OK) return rc;
    int n_cont = 0;
    for (int d = r.first; d < r.first + r.count; ++d) {
      cat |= host_labels[d].kind == TPE_JOINT_CAT;
      n_cont += host_labels[d].kind == TPE_JOINT_CONT;
    }
    if (r.n_cont != n_cont || r.g_off != dc_tot) {
      set_error("%s: group %d: n_cont=%d, g_off=%d; its labels give %d at %d", fn, g, r.n_cont,
                r.g_off, n_cont, dc_tot);
      return TPE_E_ARG;
    }
    if (n_cont > kRMaxCont) {
      set_error("%s: group %d: %d continuous labels, at most %d", fn, g, n_cont, kRMaxCont);
      return TPE_E_UNSUPPORTED;
    }
    dc_tot += n_cont;
    cond |= r.live_col >= 0;
    if (n_cont == 0 && !want_J) continue;  // (nothing of it moves and nothing is asked)
    RClass& c = cls[n_cont <= 4 ? 0 : n_cont <= 8 ? 1 : 2];
    c.g[c.n++] = g;
  }
  if (n_rows == 0 || cls[0].n + cls[1].n + cls[2].n == 0) return TPE_OK;
  if (!labels || !groups || !vals || (cat && !tables) || (cond && !active)) {
    set_error("%s: null pointer", fn);
    return TPE_E_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  launch_refine_tree<4>(cls[0], n_rows, st, labels, tables, groups, n_groups, dc_tot, vals, active,
                        ld, refine, J_start, J_end, g_end, accepted);
  launch_refine_tree<8>(cls[1], n_rows, st, labels, tables, groups, n_groups, dc_tot, vals, active,
                        ld, refine, J_start, J_end, g_end, accepted);
  launch_refine_tree<kRMaxCont>(cls[2], n_rows, st, labels, tables, groups, n_groups, dc_tot, vals,
                                active, ld, refine, J_start, J_end, g_end, accepted);
  return check_launch(fn);
}

extern "C" int64_t tpe_joint_refine_tree_stage_components(int n_labels) {
  if (n_labels < 1 || n_labels > kJMaxD) return -1;
  return stage_components(n_labels);
}

extern "C" int tpe_joint_refine_tree_group_bytes(void) { return (int)sizeof(tpe_refine_group); }
