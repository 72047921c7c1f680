// tpe_distinct.hip -- distinct configurations of a pool (tpe.distinct_rows,
// suggest_sampled / suggest_from_pool with distinct=True).
//
// Two rows hold the same configuration iff their activity bytes agree for every
// label and, for every label live in them, their values have the same
// order_key (fp64 equality with -0.0 == +0.0 and all NaNs equal); entries of
// dead labels are ignored.  For pool rows [0, P) and a list of T seen rows
// (history rows, label-major like the pool) tpe_pool_distinct writes
//
//   first[r] = -1 - t   t the smallest position of the seen list whose row holds
//                       r's configuration, if there is one; otherwise
//            = the smallest pool row that holds r's configuration,
//
// so a row is fresh (first[r] == r) iff it is the first of its class and the
// class was never seen; mask_out = taken_in | (first != r) is tpe_pool_topk's
// `taken`.
//
// Table.  An open-addressing table of cap >= 2 (P + T) slots, a power of two,
// in the caller's scratch: owner[slot] and first[slot], both int64 and both
// kEmpty (INT64_MAX) at the start.  A row's id is its pool row, or its seen
// position minus 2^62: every seen id is below every pool id and ids ascend
// with the position, so one integer minimum serves both rules above.  One
// thread per row hashes the row (a splitmix64 chain over its labels' keys, a
// dead label a fixed word), keeps the top hash_bits bits, starts at the slot
// the top bits name and probes linearly: it claims an empty slot with a 64-bit
// compare-and-swap of owner, or compares itself value by value with the
// slot's owner and moves on when they differ.  Where it stops it takes the
// integer minimum of first[slot] with its id.  Seen rows go in one launch, pool
// rows in the next, k_distinct_finish in a third.
//
// Exact: rows join a slot only after the full comparison; a hash collision
// costs probes.  Schedule-independent: owner is written once per slot, so the
// slots ahead of a row on its probe path never change their verdict, and two
// equal rows (same hash, same path) both stop at the slot either of them
// claimed first -- a class has one slot, whichever row owns it, and
// first[slot] is the minimum over the whole class.  Integer atomics only.
//
// Coherence (the XCDs' L2s are not coherent with each other): owner is decided
// by the compare-and-swap's returned value.  The relaxed agent-scope loads in
// front of the atomics only save atomics: owner is write-once, so a non-empty
// owner read there is final and an empty one is asked again by the swap;
// first only falls, so an id not below any value it ever held cannot lower it.
#include "tpe_common.hpp"

namespace tpe {
namespace {
constexpr int kDBS = 256;                       // threads per block
constexpr int64_t kEmpty = INT64_MAX;           // owner / first of an unused slot
constexpr int64_t kSeenBias = (int64_t)1 << 62; // id of seen position t: t - kSeenBias
constexpr uint64_t kDeadKey = 0;                // order_key never gives 0
constexpr int kShiftArgs = 128;                 // shifts per k_distinct_shift launch
constexpr int kShiftLabels = TPE_DISTINCT_SHIFT_LABELS;

// one side of a comparison: a pool, or the seen rows with their shifts
struct RowSet {
  const double* vals;
  const uint8_t* act;
  int64_t ld;
  const int32_t* rows;  // position -> row (seen list), or null: the identity
  const double* shift;  // device, per label below n_shift, or null
  int n_shift;
};

__device__ __forceinline__ uint64_t mix64(uint64_t h) {  // splitmix64 finaliser (tpe._mix64)
  h ^= h >> 30;
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 27;
  h *= 0x94D049BB133111EBull;
  return h ^ (h >> 31);
}

// the key of label j in row `row`: order_key of the (shifted) value, kDeadKey
// where the label is not live
__device__ __forceinline__ uint64_t entry_key(const RowSet& R, int j, int64_t row) {
  const int64_t e = (int64_t)j * R.ld + row;
  if (!R.act[e]) return kDeadKey;
  double v = R.vals[e];
  if (R.shift && j < R.n_shift) v = v - R.shift[j];
  return order_key(v);
}

__device__ __forceinline__ bool rows_equal(const RowSet& A, int64_t ra, const RowSet& B,
                                           int64_t rb, int n_labels) {
  for (int j = 0; j < n_labels; ++j)
    if (entry_key(A, j, ra) != entry_key(B, j, rb)) return false;
  return true;
}

__global__ __launch_bounds__(kDBS) void k_distinct_init(int64_t* __restrict__ tab, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kDBS + threadIdx.x;
  if (i < n) tab[i] = kEmpty;
}

struct ShiftArgs {
  double v[kShiftArgs];
};
__global__ void k_distinct_shift(ShiftArgs A, int n, double* __restrict__ out) {
  if ((int)threadIdx.x < n) out[threadIdx.x] = A.v[threadIdx.x];
}

// SEEN: thread i inserts position i of the seen list; otherwise pool row i
template <bool SEEN>
__global__ __launch_bounds__(kDBS) void k_distinct_insert(RowSet pool, RowSet seen, int64_t n,
                                                          int n_labels, int hash_bits,
                                                          int cap_bits, int64_t* owner,
                                                          int64_t* first,
                                                          int64_t* __restrict__ slot_of) {
  const int64_t i = (int64_t)blockIdx.x * kDBS + threadIdx.x;
  if (i >= n) return;
  const RowSet& mine = SEEN ? seen : pool;
  int64_t row = i;
  if (SEEN && seen.rows) {
    row = seen.rows[i];
    if (row < 0 || row >= seen.ld) return;  // not a row of the history: ignored
  }
  uint64_t h = 0x9E3779B97F4A7C15ull;
  for (int j = 0; j < n_labels; ++j) h = mix64(h ^ entry_key(mine, j, row));
  h = hash_bits == 0 ? 0 : h & (~0ull << (64 - hash_bits));
  const int64_t cap_mask = ((int64_t)1 << cap_bits) - 1;
  int64_t slot = (int64_t)(h >> (64 - cap_bits));
  const int64_t me = SEEN ? i - kSeenBias : i;
  for (;;) {
    int64_t o = __hip_atomic_load(&owner[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (o == kEmpty) {  // (a stale empty is settled by the swap: o becomes the owner it finds)
      if (__hip_atomic_compare_exchange_strong(&owner[slot], &o, me, __ATOMIC_RELAXED,
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        break;  // claimed
    }
    bool same;
    if (o < 0) {  // a seen position (all of them valid: only those are inserted)
      const int64_t t = o + kSeenBias;
      same = rows_equal(mine, row, seen, seen.rows ? (int64_t)seen.rows[t] : t, n_labels);
    } else {
      same = rows_equal(mine, row, pool, o, n_labels);
    }
    if (same) break;
    slot = (slot + 1) & cap_mask;
  }
  if (me < __hip_atomic_load(&first[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    __hip_atomic_fetch_min(&first[slot], me, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!SEEN) slot_of[i] = slot;
}

__global__ __launch_bounds__(kDBS) void k_distinct_finish(const int64_t* __restrict__ tab_first,
                                                          const int64_t* __restrict__ slot_of,
                                                          const uint8_t* __restrict__ taken_in,
                                                          int64_t n_rows,
                                                          int64_t* __restrict__ first,
                                                          uint8_t* __restrict__ mask_out) {
  const int64_t r = (int64_t)blockIdx.x * kDBS + threadIdx.x;
  if (r >= n_rows) return;
  const int64_t f = tab_first[slot_of[r]];
  const int64_t out = f < 0 ? -1 - (f + kSeenBias) : f;
  first[r] = out;
  if (mask_out) mask_out[r] = (uint8_t)((taken_in ? taken_in[r] : 0) | (out != r));
}

// log2 of the table's capacity, or -1 when it does not fit
inline int distinct_cap_bits(int64_t n_rows, int64_t n_seen) {
  if (n_rows < 0 || n_seen < 0 || n_rows > ((int64_t)1 << 56) || n_seen > ((int64_t)1 << 56))
    return -1;
  const int64_t need = 2 * (n_rows + n_seen);
  int bits = 1;
  while (((int64_t)1 << bits) < need) ++bits;
  return bits;
}
}  // namespace
}  // namespace tpe

using namespace tpe;

extern "C" int64_t tpe_pool_distinct_scratch_bytes(int64_t n_rows, int64_t n_seen) {
  const int bits = distinct_cap_bits(n_rows, n_seen);
  if (bits < 0) return -1;
  return 16 * ((int64_t)1 << bits) + 8 * n_rows + (n_seen > 0 ? 8 * (int64_t)kShiftLabels : 0);
}

extern "C" int tpe_pool_distinct(const double* vals, const uint8_t* active, int64_t ld,
                                 int64_t n_rows, int n_labels, const double* seen_vals,
                                 const uint8_t* seen_active, int64_t seen_ld,
                                 const int32_t* seen_rows, int64_t n_seen,
                                 const double* host_seen_shift, int hash_bits,
                                 const uint8_t* taken_in, int64_t* first, uint8_t* mask_out,
                                 void* scratch, void* stream) {
  const int cap_bits = distinct_cap_bits(n_rows, n_seen);
  if (cap_bits < 0 || n_labels < 0 || ld < 0 || seen_ld < 0 || hash_bits < 0 || hash_bits > 64) {
    set_error("tpe_pool_distinct: n_rows=%lld n_seen=%lld n_labels=%d ld=%lld seen_ld=%lld "
              "hash_bits=%d", (long long)n_rows, (long long)n_seen, n_labels, (long long)ld,
              (long long)seen_ld, hash_bits);
    return TPE_E_ARG;
  }
  if (n_rows == 0) return TPE_OK;  // nothing to write
  if (!first || !scratch || (n_labels > 0 && (!vals || !active)) ||
      (n_seen > 0 && n_labels > 0 && (!seen_vals || !seen_active))) {
    set_error("tpe_pool_distinct: null pointer");
    return TPE_E_ARG;
  }
  const int64_t blocks = (n_rows + kDBS - 1) / kDBS, seen_blocks = (n_seen + kDBS - 1) / kDBS;
  const int64_t cap = (int64_t)1 << cap_bits;
  if ((n_labels > 0 && ld < n_rows) || (n_labels > 0 && !seen_rows && seen_ld < n_seen) ||
      blocks > 2147483647 || seen_blocks > 2147483647 || (2 * cap + kDBS - 1) / kDBS > 2147483647) {
    set_error("tpe_pool_distinct: n_rows=%lld / n_seen=%lld do not fit ld=%lld / seen_ld=%lld / "
              "a launch", (long long)n_rows, (long long)n_seen, (long long)ld, (long long)seen_ld);
    return TPE_E_ARG;
  }
  int n_shift = 0;  // labels up to the last nonzero shift
  if (host_seen_shift && n_seen > 0)
    for (int j = 0; j < n_labels; ++j)
      if (host_seen_shift[j] != 0.0) n_shift = j + 1;
  if (n_shift > kShiftLabels) {
    set_error("tpe_pool_distinct: a nonzero shift at label %d (only the first %d labels can have "
              "one)", n_shift - 1, kShiftLabels);
    return TPE_E_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  int64_t* owner = static_cast<int64_t*>(scratch);
  int64_t* tab_first = owner + cap;
  int64_t* slot_of = tab_first + cap;
  double* shift = reinterpret_cast<double*>(slot_of + n_rows);  // (there when n_seen > 0)
  for (int j0 = 0; j0 < n_shift; j0 += kShiftArgs) {
    ShiftArgs A;
    const int n = n_shift - j0 < kShiftArgs ? n_shift - j0 : kShiftArgs;
    for (int i = 0; i < kShiftArgs; ++i) A.v[i] = i < n ? host_seen_shift[j0 + i] : 0.0;
    hipLaunchKernelGGL(k_distinct_shift, dim3(1), dim3(kShiftArgs), 0, st, A, n, shift + j0);
  }
  const RowSet pool{vals, active, ld, nullptr, nullptr, 0};
  const RowSet seen{seen_vals, seen_active, seen_ld, seen_rows, n_shift ? shift : nullptr,
                    n_shift};
  const dim3 bs(kDBS);
  hipLaunchKernelGGL(k_distinct_init, dim3((unsigned)((2 * cap + kDBS - 1) / kDBS)), bs, 0, st,
                     owner, 2 * cap);
  if (n_seen > 0)
    hipLaunchKernelGGL(k_distinct_insert<true>, dim3((unsigned)seen_blocks), bs, 0, st, pool, seen,
                       n_seen, n_labels, hash_bits, cap_bits, owner, tab_first, slot_of);
  hipLaunchKernelGGL(k_distinct_insert<false>, dim3((unsigned)blocks), bs, 0, st, pool, seen,
                     n_rows, n_labels, hash_bits, cap_bits, owner, tab_first, slot_of);
  hipLaunchKernelGGL(k_distinct_finish, dim3((unsigned)blocks), bs, 0, st, tab_first, slot_of,
                     taken_in, n_rows, first, mask_out);
  return check_launch("tpe_pool_distinct");
}
