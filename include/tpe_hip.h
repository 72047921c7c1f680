/*
 * tpe_hip.h -- C ABI of the MI355X TPE suggest engine (libtpe_hip.so).
 *
 * The reference (hyperopt 0.2.4, /root/reference) is pure Python/numpy and
 * has no FFI of its own; its hot path is the per-label posterior evaluation
 * that `tpe.suggest` drives through `pyll.rec_eval` (hyperopt/tpe.py:942).
 * Each entry point below replaces one group of the numpy expressions on that
 * path and is what a binding of that path (ctypes / cffi / pybind) would
 * call.  The Python host layer `hyperopt_amd/_lib.py` binds these with
 * ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every pointer is a caller-owned DEVICE pointer unless marked "host";
 *   - `stream` is a hipStream_t passed as void* (0 = legacy default stream);
 *   - every call is asynchronous on `stream`, captures into a hipGraph,
 *     performs no allocation and no host synchronisation;
 *   - return value: 0 on success, a negative TPE_E* code otherwise; the text
 *     of the last error on the calling thread is tpe_last_error();
 *   - scores/log-densities are float64 on the ABI; `precision` (32 or 64)
 *     selects the arithmetic of the continuous scoring kernel only.
 */
#ifndef TPE_HIP_H
#define TPE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TPE_ABI_VERSION 22

enum {
  TPE_OK = 0,
  TPE_E_ARG = -1,        /* bad argument (null pointer, bad size/kind)      */
  TPE_E_LAUNCH = -2,     /* HIP launch / runtime error                      */
  TPE_E_UNSUPPORTED = -3 /* configuration outside what the kernels support  */
};

/* mixture families (hyperopt/tpe.py:79, 229; categorical tpe.py:60-73) */
enum { TPE_GMM1 = 0, TPE_LGMM1 = 1, TPE_CAT = 2 };

/* observation transform applied before the Parzen fit (tpe.py:506-572) */
enum { TPE_OBS_IDENTITY = 0, TPE_OBS_LOG = 1 };

/* job flags */
enum {
  TPE_F_LOW = 1,        /* lower bound present (tpe.py:93, 166)              */
  TPE_F_HIGH = 2,       /* upper bound present                               */
  TPE_F_QUANT = 4,      /* quantized (q is not None)                         */
  TPE_F_INJECTED = 8,   /* candidates read from `cand` instead of sampled    */
  TPE_F_DRAW32 = 16,    /* sampled quantized job: draw in fp32 (set only when
                           every lattice index |k| <= 2^12, so fp32 resolves a
                           slot to < 2^-11 of q)                              */
  TPE_F_LATTICE_READY = 32, /* lattice job: the caller has already set its
                           slot_first region [lat_off, lat_off + lat_n) to
                           all-ones and its `counts` entry to 0 (e.g. in the
                           level's upload); when every job of a
                           tpe_lattice_sample / tpe_lattice_compact call has
                           it, those calls skip their memsets               */
  /* (TPE_F_DRAW32 on an unquantized job: the fp32 candidate stream -- the
     table path's -- scored exactly by tpe_score_pruned64)                   */
  /* The fp32 stream compares a draw against the smallest floats >= low and
     >= high, so every fp32 draw lies in [low, high) of the fp64 bounds; a
     caller should keep a label on the fp32 stream only while the fp32
     spacing at its bounds' magnitude is small against prior_sigma / 100, the
     smallest bandwidth a fit produces (the Python engine: 500 steps per
     prior_sigma).                                                           */
};

/*
 * One Parzen-fit segment: the below- or above-set observations of one label.
 * Replaces `adaptive_parzen_normal` (tpe.py:399-467) and the observation
 * transforms of the ap_*_sampler functions (tpe.py:484-572).  Inputs are set
 * by the host; the kernel fills the outputs.  The fitted mixture has
 * n_obs + 1 components written at [comp_off, comp_off + n_obs + 1), sorted
 * by mean, exactly as the reference returns them.
 */
typedef struct tpe_seg {
  /* inputs */
  int64_t obs_off;      /* first observation in the obs pool                */
  int64_t comp_off;     /* first output component in the mixture pool       */
  int32_t n_obs;        /* observations in this segment (tid order)         */
  int32_t lf;           /* linear forgetting (tpe.py:380-392); 0 = off      */
  int32_t transform;    /* TPE_OBS_*                                         */
  int32_t family;       /* TPE_GMM1 / TPE_LGMM1 (coefficient layout)         */
  double floor;         /* log transform: log(max(obs, floor))              */
  double prior_weight, prior_mu, prior_sigma;
  double low, high;     /* truncation for p_accept (tpe.py:145-150)         */
  int32_t bounded;      /* 1 if low/high given                              */
  /* outputs */
  int32_t prior_pos;    /* index of the prior component in the sorted mix   */
  double p_accept;      /* sum w*(Phi(high)-Phi(low)), 1 if unbounded        */
  double cmax;          /* max_k log2-coefficient (fp32 scoring offset)      */
  double center;        /* fp32 scoring origin (float-rounded prior_mu)      */
  double lglob;         /* lower bound of log2(sum)-cmax over the support    */
  int32_t n_wide;       /* wide components (prior + sigma >= sigma_p/4)      */
  int32_t given;        /* 1: an explicit mixture (tpe_mixture_prepare): its
                           w / mu / sigma are the caller's, not fitted       */
} tpe_seg;

/*
 * One categorical segment (randint / pchoice / choice posterior,
 * tpe.py:578-615 with pyll/base.py:1053-1060).  counts are accumulated in
 * observation order, so they are bit-identical to np.bincount.
 */
typedef struct tpe_cat_seg {
  int64_t obs_off;      /* int64 observations (already offset-free)         */
  int64_t p_off;        /* first output probability                          */
  int32_t n_obs;
  int32_t n_cat;        /* K                                                 */
  int32_t lf;
  int32_t mode;         /* 0 randint: counts+pw ; 1 categorical: counts+K*pw*p */
  double prior_weight;
  int64_t prior_p_off;  /* mode 1: prior probabilities p in the p pool       */
} tpe_cat_seg;

/*
 * One label's scoring job.  For continuous labels below/above index two
 * tpe_seg entries; for categorical labels two tpe_cat_seg entries.
 * Candidates are either sampled in registers from the BELOW posterior with
 * Philox4x32-10 keyed by (key, global candidate index) -- so results do not
 * depend on how candidates are sharded over GPUs -- or injected (TPE_F_INJECTED).
 */
typedef struct tpe_job {
  int32_t family;       /* TPE_GMM1 / TPE_LGMM1 / TPE_CAT                    */
  int32_t flags;        /* TPE_F_*                                           */
  int32_t below, above; /* segment indices                                   */
  double low, high, q;  /* GMM1: x-space bounds; LGMM1: log-space bounds    */
  int64_t n_cand;       /* candidates scored by this call                   */
  int64_t cand_base;    /* global index of the first one (multi-GPU shard)  */
  int64_t cand_off;     /* TPE_F_INJECTED: first candidate in `cand`         */
  uint64_t key;         /* Philox key (seed mixed with label id)            */
  int64_t lat_off;      /* quantized: first lattice slot in the slot pool   */
  int64_t lat_kmin;     /* quantized: lattice index of slot 0               */
  int64_t lat_n;        /* quantized: number of slots; categorical: K (0 = unknown) */
  int64_t out_off;      /* optional per-candidate outputs: first element    */
  double bin_lo, bin_hi;/* sorted path: candidate coordinate range to bin    */
  int64_t sort_off;     /* sorted path: first slot in the sorted pool        */
  int64_t cnt_off;      /* sorted path: first element of the count matrix    */
  int64_t tbl_off;      /* table path: first cell of this job's cell table   */
  int64_t tbl_cap;      /* table path: cells allocated at tbl_off            */
} tpe_job;

/* best candidate of one label: np.argmax semantics (first max, NaN wins) */
typedef struct tpe_best {
  double score;         /* below_llik - above_llik of the winner            */
  int64_t index;        /* global candidate index of the winner (-1: none)  */
  double value;         /* candidate value (category index for TPE_CAT)     */
  int64_t n_scored;     /* candidates entered into the argmax               */
} tpe_best;

/* ---- Parzen posterior (adaptive_parzen_normal, tpe.py:399-467) ---------- */
/* obs: fp64 pool (n_obs_total); scratch: device workspace of
 * tpe_fit_scratch_bytes(n_seg, max_obs, n_obs_total) bytes;
 * w/mu/sigma: fp64 mixture pool (sorted components);
 * wcdf: fp64 cumulative weights (sampler); coef64: 4 doubles / component;
 * coef32: 4 floats / component.  max_obs = max n_obs over segs.
 * Pruning data for the sorted scoring path (per component, float; all four
 * NULL to skip): coef32n = coef32 with wide components masked (c = -inf),
 * wide32 = the wide components' coefficients compacted at comp_off, pm / sm
 * = prefix max of (mu + reach) / suffix min of (mu - reach) over narrow
 * components. */
int64_t tpe_fit_scratch_bytes(int n_seg, int max_obs, int64_t n_obs_total);
int tpe_parzen_fit(const double* obs, void* scratch, tpe_seg* segs, int n_seg, int max_obs,
                   int64_t n_obs_total, double* w, double* mu, double* sigma, double* wcdf,
                   double* coef64, float* coef32, float* coef32n, float* wide32, float* pm,
                   float* sm, void* stream);

/* ---- observation lists from an HBM-resident history ---------------------
 * Replaces the per-suggest rebuild of miscs_to_idxs_vals (base.py:200-214)
 * and the list comprehensions of ap_split_trials (tpe.py:623-646, tid order
 * kept).  vals / active: label-major matrices, element (col, row) at
 * col * ld + row; rows (nullable = identity): the n_rows history rows in tid
 * order; is_below: one flag per position of `rows` (1 = among the n_below
 * best losses).  Each descriptor compacts the rows active for `col` on its
 * side of the split into obs_f64 (Parzen fit pool) or, with to_int, into
 * obs_i64 as (int64)value - offset (categorical pool), writing at most
 * `count` elements; a different number of matches sets bit 4 of *err. */
typedef struct tpe_gather {
  int32_t col;          /* label column                                      */
  int32_t below;        /* 1: below rows, 0: above rows                      */
  int64_t dst_off;      /* first output element                              */
  int64_t offset;       /* to_int: subtracted (randint low)                  */
  int64_t count;        /* elements expected (the segment's n_obs)           */
  int32_t to_int;       /* 1: int64 output, 0: fp64 output                   */
  int32_t hist;         /* tpe_gather_obs_multi: index of the history (else 0) */
} tpe_gather;
/* Rows appended to an HBM-resident history: `stage` (device) holds the new
 * rows' values, label-major (n_labels x k fp64), then their active flags
 * (n_labels x k bytes); they are written to rows r0..r0+k-1 of vals / active
 * (label-major, leading dimension ld). */
int tpe_history_append(const void* stage, int n_labels, int64_t k, double* vals, uint8_t* active,
                       int64_t ld, int64_t r0, void* stream);
int tpe_gather_obs(const double* vals, const uint8_t* active, int64_t ld, const int32_t* rows,
                   int64_t n_rows, const uint8_t* is_below, const tpe_gather* gathers,
                   const tpe_gather* host_gathers, int n_gathers, double* obs_f64,
                   int64_t* obs_i64, int32_t* err, void* stream);

/* Many histories in one launch (batched independent studies, the C4 shape of
 * SURVEY §8(f) row 3): gather g reads history hists[g.hist].  A history's
 * row list (rows_off < 0: identity) and split flags live in the caller's
 * `aux` buffer at byte offsets rows_off / isb_off; n_cols bounds `col`. */
typedef struct tpe_history {
  const double* vals;     /* label-major values, (col, row) at col * ld + row    */
  const uint8_t* active;  /* same layout, 1 = label active in that row          */
  int64_t ld;
  int64_t n_cols;
  int64_t n_rows;         /* positions (length of the row list / flags)         */
  int64_t rows_off;       /* byte offset of int32 rows in aux, or -1 (identity) */
  int64_t isb_off;        /* byte offset of the uint8 split flags in aux        */
} tpe_history;
int tpe_gather_obs_multi(const tpe_history* hists, const tpe_history* host_hists, int n_hists,
                         const void* aux, const tpe_gather* gathers,
                         const tpe_gather* host_gathers, int n_gathers, double* obs_f64,
                         int64_t* obs_i64, int32_t* err, void* stream);

/* ---- sorted history: the Parzen fit without a per-suggest sort ------------
 * adaptive_parzen_normal (tpe.py:399-467) sorts each below / above set; both
 * are subsets of the label's history, and a stable sort of a subset is the
 * history's stable order with the other rows left out.  The history keeps,
 * for every fitted column, its rows sorted by (transformed value, row) in
 * `order` (label-major like vals: column col's order at order + col * ld);
 * tpe_history_order merges rows [n_old, n_old + n_new) (n_new <= 2048 per
 * call) into the order of rows [0, n_old) -- O(rows) per append.  The
 * transform is the fit's: log(max(v, floor)) for TPE_OBS_LOG (NaN last).
 * scratch: tpe_history_order_scratch_bytes(n_specs, n_old + n_new) bytes. */
typedef struct tpe_colspec {
  int32_t col;          /* history column                                    */
  int32_t transform;    /* TPE_OBS_*                                         */
  double floor;         /* TPE_OBS_LOG: log(max(v, floor))                   */
} tpe_colspec;
int64_t tpe_history_order_scratch_bytes(int n_specs, int64_t n_rows);
int tpe_history_order(const double* vals, int64_t ld, const tpe_colspec* specs,
                      const tpe_colspec* host_specs, int n_specs, int64_t n_old, int64_t n_new,
                      int32_t* order, void* scratch, void* stream);
/* The fit of segment i (segs[i]) from the sorted history: gathers[i] names its
 * column, side (below: 1) and observation count (identity row list: row r of
 * the history is position r, is_below[r] its split flag, n_rows of them).
 * A chunked compaction, one block per (chunk of rows, segment), in two
 * launches (three for very long columns): first the rows in tid order -- per
 * chunk the member count, how many members lie below the prior mean (its
 * searchsorted slot), the first member row, and every row's rank among its
 * chunk's members (the linear-forgetting positions once the chunk bases are
 * added) --, then the column's order compacted to the segment (means and
 * weights in sorted order); then tpe_parzen_fit's own bandwidth /
 * coefficient launches (same bits).  A count other than gathers[i].count
 * sets bit 4 of *err: nothing of that segment is written, neither to the
 * pools nor to segs[i] (the bandwidth / coefficient launches skip it), and
 * the call's results are void.
 * Precondition: `order` holds, per column, a permutation of the rows
 * [0, n_rows) -- n_rows must be the history's row count (tpe_history_order's
 * n_rows), so is_below must hold exactly one flag per history row.
 * scratch: tpe_fit_sorted_scratch_bytes(n_seg, n_rows) bytes.
 *
 * tpe_fit_sorted_layout (host only, no GPU call): where a call with these
 * (n_seg, n_rows) keeps its intermediate state in `scratch`, which is still
 * there when the call has ended, and the sizes the history kernels cut their
 * work by.  Writes up to n of these nine numbers to out and returns how many
 * it wrote (-1: bad arguments):
 *   [0] byte offset of the rank words, one int32 per (segment, row) at
 *       segment * n_rows + row: -1 for a row that is not a member, else the
 *       row's rank among the members of its chunk of out[4] rows (its
 *       position in the segment's whole tid-ordered list where the globalize
 *       path ran),
 *   [1] byte offset of the chunk counts, out[5] int32 per (segment, chunk) at
 *       segment * chunks + chunk: members in the chunk of rows, how many of
 *       them have a key below the prior mean's, the first member row
 *       (INT32_MAX: none), members in the same chunk of the sorted order,
 *   [2] byte offset of the fit tail's partials (after them, up to the total,
 *       one int32 per segment: 1 where the count differed),
 *   [3] the total, tpe_fit_sorted_scratch_bytes(n_seg, n_rows),
 *   [4] rows per chunk, [5] ints per count record,
 *   [6] the chunk count above which the ranks are globalized in a launch of
 *       their own,
 *   [7] positions per pass of tpe_gather_obs / tpe_gather_obs_multi,
 *   [8] the most new rows one tpe_history_order call takes. */
int64_t tpe_fit_sorted_scratch_bytes(int n_seg, int64_t n_rows);
int tpe_fit_sorted_layout(int n_seg, int64_t n_rows, int64_t* out, int n);
int tpe_fit_sorted(const double* vals, const uint8_t* active, int64_t ld, const int32_t* order,
                   int64_t n_rows, const uint8_t* is_below, const tpe_gather* gathers,
                   const tpe_gather* host_gathers, tpe_seg* segs, int n_seg, void* scratch,
                   double* w, double* mu, double* sigma, double* wcdf, double* coef64,
                   float* coef32, int32_t* err, void* stream);

/* ---- explicit mixtures (GMM1 / LGMM1 with given parameters) -------------
 * The reference's GMM1 / GMM1_lpdf / LGMM1 / LGMM1_lpdf (tpe.py:79-180,
 * 229-307) take the mixture directly (weights, mus, sigmas, low, high, q).
 * tpe_mixture_prepare readies such mixtures for tpe_sample and the scorers:
 * every segment (given = 1) holds its K = n_obs + 1 components at comp_off in
 * w (raw weights) / mu / sigma, prior_pos any component index, prior_mu a
 * point near the mixture (the fp32 coefficients' origin), low / high /
 * bounded its truncation.  Writes the normalised weights, p_accept (GMM1),
 * the cumulative weights and the fp64 / fp32 coefficients exactly as the fit
 * does for a fitted mixture (the sigmas are kept as given).
 * scratch: tpe_mixture_scratch_bytes(n_seg, max_comp) bytes. */
int64_t tpe_mixture_scratch_bytes(int n_seg, int max_comp);
int tpe_mixture_prepare(tpe_seg* segs, int n_seg, int max_comp, void* scratch, double* w,
                        const double* mu, double* sigma, double* wcdf, double* coef64,
                        float* coef32, void* stream);

/* ---- categorical posterior (tpe.py:578-615) ------------------------------ */
/* p_pool: probabilities (mode 1 also reads the prior p from it at
 * prior_p_off); logp_pool / cdf_pool: log p and cumulative p at p_off.
 * max_cat: the largest n_cat over segs (host value, sizes the grid). */
int tpe_cat_posterior(const int64_t* obs, const tpe_cat_seg* segs, int n_seg, int max_cat,
                      double* p_pool, double* logp_pool, double* cdf_pool, void* stream);

/* The same posteriors read straight from an HBM-resident history (the
 * arguments of tpe_gather_obs below): segment i's observations are the rows
 * of column gathers[i].col active there and on side gathers[i].below of the
 * split (is_below; rows: optional row list), in row order, their category
 * (int64)value - gathers[i].offset -- the lists tpe_gather_obs would write,
 * counted without writing them.  gathers: device array aligned with segs
 * (obs_off unused).  An observation count other than segs[i].n_obs sets bit
 * 4 of *err.  Replaces tpe_gather_obs + tpe_cat_posterior for the
 * categorical labels of a level (tpe.py:578-615, pyll/base.py:1053-1060).
 * work (device, nullable) of work_bytes >= tpe_cat_hist_scratch_bytes(n_seg,
 * max_cat, n_rows) > 0: a long history is counted in row chunks by many
 * blocks (the same bits); otherwise one block per (segment, category). */
int tpe_cat_posterior_hist(const double* vals, const uint8_t* active, int64_t ld,
                           const int32_t* rows, int64_t n_rows, const uint8_t* is_below,
                           const struct tpe_gather* gathers, const tpe_cat_seg* segs, int n_seg,
                           int max_cat, double* p_pool, double* logp_pool, double* cdf_pool,
                           void* work, int64_t work_bytes, int32_t* err, void* stream);
/* Work bytes of tpe_cat_posterior_hist's chunked path for these sizes (0:
 * the sizes take the single-block path; -1: bad arguments). */
int64_t tpe_cat_hist_scratch_bytes(int n_seg, int max_cat, int64_t n_rows);

/* ---- continuous candidates: sample (or read) + score + argmax ------------
 * Replaces GMM1/LGMM1 sampling (tpe.py:79-106, 229-257), GMM1_lpdf /
 * LGMM1_lpdf (tpe.py:117-180, 265-307) and broadcast_best (tpe.py:649-658)
 * for UNQUANTIZED labels.  partial: workspace of tpe_best, capacity
 * n_partial (query with tpe_score_partials()).  out_bl/out_al (nullable):
 * per-candidate log-likelihoods at job.out_off; out_x (nullable): the
 * candidates themselves.  best: one tpe_best per job. */
int64_t tpe_score_partials(const tpe_job* host_jobs, int n_jobs);
int tpe_score_continuous(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                         const tpe_seg* segs, const double* w, const double* mu,
                         const double* sigma, const double* wcdf, const double* coef64,
                         const float* coef32, const double* cand, int precision,
                         double* out_bl, double* out_al, double* out_x,
                         tpe_best* partial, int64_t n_partial, tpe_best* best,
                         void* stream);

/* ---- continuous candidates, sorted + pruned (fp32 throughput path) -------
 * Same results as tpe_score_continuous(precision=32) on sampled candidates
 * (same Philox draws, same winner up to fp32 rounding), but candidates are
 * first bucketed by value (count -> scan -> scatter, deterministic, no
 * global atomics) so each scoring block spans a narrow interval and only
 * components within reach -- those whose term can exceed 2^-40 of the
 * mixture sum -- plus the wide components are evaluated.
 * tpe_sort_layout: count-matrix elements and sorted-pool slots one job of
 * n_cand candidates needs.  pairs (nullable): u64 counter of evaluated
 * (candidate, component) pairs. */
int64_t tpe_sort_layout(int64_t n_cand, int64_t* sorted_slots);
/* draw the candidates (same Philox streams as tpe_score_continuous) into
 * gen (generation order) and bucket them by value into sorted_x / sorted_i
 * (candidate value, local index); gen/sorted at job.sort_off, counts: a
 * workspace of 2 x tpe_sort_layout() elements per job at 2 * job.cnt_off */
int tpe_sort_candidates(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                        const tpe_seg* segs, const double* mu, const double* sigma,
                        const double* wcdf, uint32_t* counts, float* gen,
                        float* sorted_x, uint32_t* sorted_i, void* stream);
/* score the bucketed candidates with component pruning + fused argmax */
int tpe_score_sorted(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                     const tpe_seg* segs, const float* coef32, const float* coef32n,
                     const float* wide32, const float* pm, const float* sm,
                     const float* sorted_x, const uint32_t* sorted_i,
                     tpe_best* partial, int64_t n_partial, tpe_best* best,
                     uint64_t* pairs, void* stream);

/* ---- continuous candidates, cell-table path (fp32 throughput path) -------
 * Same quantity as tpe_score_continuous(precision=32): per candidate the log
 * densities of both mixtures (GMM1_lpdf / LGMM1_lpdf, tpe.py:117-180,
 * 265-307) and the fused argmax (broadcast_best, tpe.py:649-658).  The
 * candidate coordinate range is cut into nb cells of half-width h.  On every
 * cell each mixture sum_j exp(l_j(y)) is expanded around the cell centre y0
 * as exp(m) * sum_{n<9} P_n u^n, u = (y - y0)/h: a degree-8 polynomial whose
 * P_0..P_5 are stored in fp32 and P_6..P_8 in fp16 (tpe_table_build).  Each
 * component's factor exp(A u + B u^2) is expanded only where 9|A| + 65|B| <=
 * 5.8 (series truncation <= 4.4e-7 relative on |u| <= 1.0501,
 * tools/table_bounds.py); the stored polynomial's whole error against its
 * mixture -- truncation, the build's fp32 terms, series, sums and merges,
 * fp32/fp16 storage -- is bounded per job from the build's worst case
 * (tpe_table.eps_mix); components whose largest term
 * on the whole range is below e^-17 / M of the prior component's smallest
 * term are left out (together < 4.2e-8 of the sum, a term of eps_mix).
 * From those two polynomials the build also fits, per cell, a cubic of the
 * score f(u) = (m_b - m_a) + log P_b(u) - log P_a(u) at four Chebyshev nodes
 * of [-1.05, 1.05], rounds it to fp32 and BOUNDS its error against f on
 * |u| <= 1.0501 (per sub-interval, the log series of both polynomials and a
 * majorant of its remainder): a cell whose bound exceeds 1e-6 is flagged;
 * the largest bound of the others (with the cubic's evaluation terms) is
 * tpe_table.eps_cubic.
 * A candidate whose cell fails the bound, or that lies outside the grid, is
 * scored by the exact fp32 log-sum-exp over all components instead.
 * tables: one tpe_table per job (device); cells: byte pool, 128 B per cell
 * slot: job j's region starts at 128 * job.tbl_off and holds tbl_cap 64-B
 * cells, then tbl_cap (m_below, m_above) fp32 pairs, then (at the next 16-B
 * boundary) tbl_cap 16-B score cubics {c0, c1, c2, c3} (c0 NaN: flagged);
 * reach_hi / reach_lo: fp64 per-component workspace (size of the mixture
 * pool); wide_idx: int32, same size.
 * stats (nullable, 3 x u64): [0] candidates scored by a fallback (exact
 * log-sum-exp; for tpe_score_table_fast also the two-polynomial cell),
 * [1] cells that failed the bound, [2] score cubics that failed their check. */
typedef struct tpe_table {
  double lo, hi;        /* candidate coordinate range (x, or log x for LGMM1) */
  double h_below, h_above; /* largest admissible half-width per mixture       */
  double origin;        /* left edge of cell 0 (cell c is centred at         */
                        /* origin + (2c+1) h)                                */
  double h;             /* cell half-width used                              */
  float inv_h, inv_w;   /* 1/h and 1/(2h)                                    */
  int32_t nb;           /* cells used (<= job.tbl_cap)                       */
  int32_t n_wide_below, n_wide_above;
  float slope;          /* max over unflagged cells of |c1| + 2.11|c2| + 3.31|c3|:
                           a bound of |df/du| on |u| <= 1.0501 (score cubics),
                           written by tpe_table_build                        */
  float eps_cubic;      /* max over unflagged cells of the proven bound of
                           |s32 - f^(u)| for a cubic-scored candidate, less its
                           2^-22 |s32| part: the cubic's fit to the stored
                           polynomials' score f^ (interval remainder, DESIGN.md
                           3.1), its fp32 evaluation and u's rounding, and the
                           fp32 score offset                                  */
  float eps_mix;        /* proven bound of the relative error of one stored
                           polynomial against its mixture on |u| <= 1.0501
                           (truncation, exclusion, the build's fp32 terms,
                           series, sums and merges, fp32/fp16 storage)       */
  int32_t build_items;  /* most components one cell's expansion summed       */
  float build_ab;       /* max over summed components of 1.0501|A| + 1.1028|B| */
  double T_below, T_above; /* log-term floor: components whose term stays
                              below it on a cell are left out               */
} tpe_table;

/* partial-workspace entries tpe_score_table needs */
int64_t tpe_table_partials(const tpe_job* host_jobs, int n_jobs);
/* scratch: tpe_table_scratch_bytes(n_jobs, max_comp) bytes; max_comp = the
 * largest component count (n_obs + 1) of the jobs' mixtures */
int64_t tpe_table_scratch_bytes(int n_jobs, int max_comp);
int tpe_table_build(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                    const tpe_seg* segs, const double* mu, const double* sigma,
                    const double* coef64, int max_comp, double* reach_hi, double* reach_lo,
                    int32_t* wide_idx, double* scratch, tpe_table* tables, float* cells,
                    uint64_t* stats, void* stream);
int tpe_score_table(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                    const tpe_seg* segs, const double* mu, const double* sigma,
                    const double* wcdf, const float* coef32, const tpe_table* tables,
                    const float* cells, const double* cand, double* out_bl, double* out_al,
                    double* out_x, tpe_best* partial, int64_t n_partial, tpe_best* best,
                    uint64_t* stats, void* stream);
/* The suggest path (sampled jobs only), in two calls.
 * tpe_score_table_fast: the same draws as tpe_score_table; each candidate is
 * scored by its cell's score cubic -- one 16-B load and three FMAs -- or, on a
 * flagged cubic, by the two-polynomial cell, then the exact fp32
 * log-sum-exp.  Writes the per-block fp32 winners to `partial` and the band
 * tiles.  tpe_band_rescore: the winner decided EXACTLY -- np.argmax
 * (tpe.py:649-658) over the fp64 scores of every candidate that can still be
 * the maximum.
 *
 * Band.  With eps(s) a proven bound of |s32 - s64| (for a
 * cubic-scored candidate eps = table.eps_cubic + 2.0001 table.eps_mix +
 * 2^-22 |s32|; a two-polynomial candidate carries its own; a log-sum-exp
 * candidate is always re-scored), candidate i can be the exact winner only if
 * s32_i + eps_i >= G := max_k (s32_k - eps_k).  Each scorer block (tile of
 * 8192 candidates) writes, without atomics, a header {lo = its best
 * s32 - eps, hi_max = its largest s32 + eps, n} (4 uint32 per tile in
 * band_ctl) and its candidates with s32 + eps >= lo (a superset: G >= lo)
 * into its own 256 entries of `band` (n = 0xFFFFFFFF: more than tile_cap,
 * <= 256, did not fit; tests shrink tile_cap to force the overflow path).
 * tpe_band_rescore (one launch, 4 blocks per job) takes G from the headers,
 * keeps the entries with s32 + eps >= G and re-scores them in fp64 -- per
 * table cell, a degree-20 expansion of both mixtures around the cell centre
 * over every component within e^-45 of the sum (components whose series
 * would converge slowly summed term by term) -- and takes the np.argmax
 * winner (largest score, then smallest index): best[j] = {fp64 score, index,
 * value (x, or exp(y) in fp64 for LGMM1), n_cand}.  A job with a full tile
 * that can still hold the winner (hi_max >= G) keeps the fp32 winner with
 * n_scored = -1: the caller re-scores it exactly (tpe_score_pruned64 with
 * TPE_F_DRAW32).
 * band / band_ctl / work: tpe_band_bytes(host_jobs, n_jobs, &ctl, &work),
 * ctl and work bytes (work: zeroed once before its first use; the rescore
 * leaves it zero).  No state carries from one call to the next in band or
 * band_ctl: every tile rewrites its header.  Both calls take the same job
 * list and partial workspace (tpe_table_partials()).
 * out_score / out_x / out_eps (nullable, tests): per candidate at
 * job.out_off, the fp32 score, the value and the bound eps used (+inf for
 * a log-sum-exp candidate). */
typedef struct tpe_band {
  int64_t index;        /* global candidate index                            */
  float y;              /* candidate in the scoring coordinate (fp32 draw)   */
  float hi;             /* s32 + eps: upper bound of its exact score          */
} tpe_band;
int64_t tpe_band_bytes(const tpe_job* host_jobs, int n_jobs, int64_t* ctl_bytes,
                       int64_t* work_bytes);
int tpe_score_table_fast(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                         const tpe_seg* segs, const double* mu, const double* sigma,
                         const double* wcdf, const float* coef32, const tpe_table* tables,
                         const float* cells, tpe_band* band, uint32_t* band_ctl,
                         double* out_score, double* out_x, double* out_eps, tpe_best* partial,
                         int64_t n_partial, int tile_cap, uint64_t* stats, void* stream);
int tpe_band_rescore(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                     const tpe_seg* segs, const double* coef64, const tpe_table* tables,
                     const tpe_band* band, const uint32_t* band_ctl, const tpe_best* partial,
                     int64_t n_partial, tpe_best* best, void* work, void* stream);
/* tpe_band_layout (host only, tests): the first n of the band work's layout
 * and the two stages' constants to out; returns how many there are (19):
 * bytes of one job's work; byte offsets in it of ns, ncell, over, direct
 * (int32), sy (float[]), sidx (int64[]), cells (int32[]); then blocks per
 * job, direct survivors (always / at most), listed cells, survivors, tiles,
 * slow components per list, entries per tile, candidates per tile, header
 * words per tile, and the "tile full" count. */
int tpe_band_layout(int64_t* out, int n);

/* ---- continuous candidates, exact fp64 with pruning (parity mode) ----------
 * Same results as tpe_score_continuous(precision=64) up to fp64 rounding (a
 * sampled job with TPE_F_DRAW32 scores the fp32 stream of the table path
 * instead -- the exact re-score of a job whose band overflowed): the
 * plan of tpe_table_build (with an e^-40 exclusion margin and the fp64
 * sampler's |z| < 8.7 range) finds, per mixture, the components whose term
 * can reach e^-40 of the sum somewhere on the candidate range, with reach
 * windows over the sorted means; each candidate sums its window plus the
 * wide components in fp64 (every component when it lies off the range), so
 * the work per candidate follows the components near it, not M.  Workspaces
 * as tpe_table_build (reach_hi / reach_lo / wide_idx / scratch / tables);
 * partial: tpe_pruned64_partials() entries.  out_* as tpe_score_continuous. */
int64_t tpe_pruned64_partials(const tpe_job* host_jobs, int n_jobs);
int tpe_score_pruned64(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                       const tpe_seg* segs, const double* mu, const double* sigma,
                       const double* wcdf, const double* coef64, int max_comp,
                       double* reach_hi, double* reach_lo, int32_t* wide_idx, double* scratch,
                       tpe_table* tables, const double* cand, double* out_bl, double* out_al,
                       double* out_x, tpe_best* partial, int64_t n_partial, tpe_best* best,
                       void* stream);

/* ---- quantized labels: lattice path ---------------------------------------
 * Candidates of a quantized label take values k*q (np.round(x/q)*q,
 * tpe.py:106, 256); equal values have equal scores, so every distinct value
 * is scored once (fp64, the reference's erf-pair sum) and the argmax keeps the
 * first candidate index of the best value -- identical to np.argmax over all
 * candidates.  slot_first: uint64 pool of lattice slots (all jobs);
 * vals/firsts/scores: compacted present values (capacity n_cap per job at
 * job.lat_off); counts: int64 per job. */
int tpe_lattice_sample(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                       const tpe_seg* segs, const double* mu, const double* sigma,
                       const double* wcdf, uint64_t* slot_first, int32_t* err,
                       void* stream);
int tpe_lattice_compact(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                        const uint64_t* slot_first, double* vals, int64_t* firsts,
                        int64_t* counts, void* stream);
/* scores values (lattice values, or injected candidates when firsts==NULL
 * and counts==NULL: then job.n_cand values at job.cand_off of `vals`).
 * err: int32 flag set to 1 on a negative lognormal_cdf argument
 * (tpe.py:196-197). */
int64_t tpe_quantized_partials(const tpe_job* host_jobs, int n_jobs, int64_t max_vals);
/* reach_hi / reach_lo (nullable, both or neither): scratch of one double per
 * component of the pools (indexed by comp_off like the table path's): the
 * prefix max of mu + b / suffix min of mu - b, b = 6.5 max(sqrt2 sigma, EPS),
 * of every job's two mixtures (written here, k_qreach), so each value sums
 * only the window of components whose erf pair is not saturated -- the same
 * sums bit for bit as the full loop (NULL). */
int tpe_score_quantized(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                        const tpe_seg* segs, const double* w, const double* mu,
                        const double* sigma, const double* vals, const int64_t* firsts,
                        const int64_t* counts, int64_t max_vals, double* out_bl,
                        double* out_al, tpe_best* partial, int64_t n_partial,
                        tpe_best* best, int32_t* err, double* reach_hi, double* reach_lo,
                        void* stream);
/* The suggest path's lattice argmax, prefix first (replaces sample + compact
 * + score + reduce for sampled jobs without per-candidate outputs; the
 * result is the same tpe_best).  Draws the first `prefix` candidates of every
 * job (a positive multiple of 4096), scores every lattice slot, and takes the
 * best seen value at its first index; a job where a slot not yet seen scores
 * higher (or NaN) draws the rest of its stream and decides again.  A value
 * first seen after the prefix can only win by a strictly better score, so
 * the winner is np.argmax's over the whole stream either way.
 * partial: >= n_jobs * max(lat_n) tpe_best; need: int32 per job (written). */
int tpe_lattice_suggest(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                        const tpe_seg* segs, const double* w, const double* mu,
                        const double* sigma, const double* wcdf, uint64_t* slot_first,
                        int64_t prefix, tpe_best* partial, int64_t n_partial, int32_t* need,
                        tpe_best* best, int32_t* err, double* reach_hi, double* reach_lo,
                        void* stream);  /* reach_hi / reach_lo: as tpe_score_quantized */

/* ---- categorical labels: sample (or read) + score + argmax ---------------- */
int64_t tpe_categorical_partials(const tpe_job* host_jobs, int n_jobs);
int tpe_score_categorical(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                          const tpe_cat_seg* csegs, const double* logp_pool,
                          const double* cdf_pool, const double* cand, double* out_bl, double* out_al,
                          double* out_x, tpe_best* partial, int64_t n_partial,
                          tpe_best* best, void* stream);
/* The suggest path's categorical argmax, prefix first (sampled jobs without
 * per-candidate outputs; the same tpe_best as tpe_score_categorical).  Draws
 * the first `prefix` candidates of every job (a positive multiple of 4096);
 * a later candidate can only win with a strictly better-scoring category, all
 * of which are then absent from the prefix -- a job where one of them can be
 * drawn at all (non-empty inverse-CDF interval) draws the rest of its stream
 * and decides again.  partial: >= tpe_categorical_partials(); need: int32
 * per job (written: 1 = the rest was drawn). */
int tpe_categorical_suggest(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
                            const tpe_cat_seg* csegs, const double* logp_pool,
                            const double* cdf_pool, int64_t prefix, tpe_best* partial,
                            int64_t n_partial, int32_t* need, tpe_best* best, void* stream);

/* ---- sampler only (KS tests, debugging): n_cand draws of job.below ------- */
int tpe_sample(const tpe_job* jobs, const tpe_job* host_jobs, int n_jobs,
               const tpe_seg* segs, const double* mu, const double* sigma,
               const double* wcdf, int precision, double* out_x, void* stream);

/* ---- prior draws (startup phase: rand.suggest, hyperopt/rand.py:15-27) ----
 * Replaces the prior samplers of pyll/stochastic.py:36-158: n draws of every
 * prior, draw i of prior j at out[j * n + i], a function of (key, base + i)
 * only (Philox4x32-10).  kind: TPE_PRIOR_*; a, b = low, high (uniform,
 * loguniform in log space, randint: [low, high)) or mu, sigma (normal,
 * lognormal in log space); q > 0 quantizes as np.round(x / q) * q;
 * categorical: n_cat probabilities at p + p_off (need not be normalised).
 * Values are fp64 (category / randint values as whole numbers). */
enum {
  TPE_PRIOR_UNIFORM = 0, TPE_PRIOR_LOGUNIFORM = 1, TPE_PRIOR_NORMAL = 2,
  TPE_PRIOR_LOGNORMAL = 3, TPE_PRIOR_RANDINT = 4, TPE_PRIOR_CATEGORICAL = 5
};
typedef struct tpe_prior {
  int32_t kind;
  int32_t n_cat;        /* categorical: number of categories                 */
  double a, b, q;
  int64_t p_off;        /* categorical: first probability in `p`             */
  uint64_t key;         /* Philox key (seed mixed with the label)            */
} tpe_prior;
int tpe_prior_sample(const tpe_prior* priors, const tpe_prior* host_priors, int n_priors,
                     const double* p, int64_t n, int64_t base, double* out, void* stream);

/* ---- annealing (anneal.suggest, hyperopt/anneal.py:100-391) ----------------
 * One level of the annealing walk for n_trials new trials against one
 * HBM-resident history (vals / active / ld / n_rows as tpe_gather_obs; loss:
 * one fp64 per history row, +inf for an unfinished trial, NaN sorts last).
 * One block per new trial visits its live labels in order (CSR: trial t's
 * items are item_label[item_off[t] .. item_off[t + 1]), indices into recs;
 * n_items = item_off[n_trials]).  Per label: the first row of the trial's
 * chain (chain + t * chain_ld, chain_n[t] rows; rows chosen at earlier labels
 * and levels -- the caller zeroes chain_n before the first level) where the
 * label is active is reused; otherwise g = geometric(1 / avg_best_idx) - 1,
 * clipped to [0, n_active - 1], picks the row of rank g among the column's
 * active rows in np.argsort(loss, kind="stable") order (ascending, NaN after
 * +inf, ties to the earlier row) by a radix select over the loss bits -- no
 * sort -- and that row joins the chain.  The value is then drawn from the
 * label's prior concentrated around the row's value by `shrink` (uniform
 * kinds: half-width 0.5 (b - a) shrink around the clipped value; normal
 * kinds: sigma b shrink; randint / categorical: (1 - shrink) onehot + shrink
 * prior).  A record with n_active == 0 draws from its prior as
 * tpe_prior_sample does.  Philox4x32-10 keyed by (key, new_ids[t]); the pick
 * and the value use separate counters.
 * out: one fp64 per item (randint: the value itself, low included).
 * dbg (nullable): one record per item.  err: bit 4 is set when the kernel
 * counts another number of active rows than rec.n_active (the pick is then
 * clipped to the rows found), bit 8 on an item list or chain out of range. */
typedef struct tpe_anneal {
  int32_t kind;         /* TPE_PRIOR_*                                       */
  int32_t n_cat;        /* categorical: number of categories                 */
  double a, b, q;       /* as tpe_prior                                      */
  int64_t p_off;        /* categorical: first prior probability in `p`       */
  uint64_t key;         /* Philox key (seed mixed with the label)            */
  int32_t col;          /* history column                                    */
  int32_t n_active;     /* host's count of the column's active rows          */
  double shrink;        /* 1 / (1 + n_active * shrink_coef)                  */
} tpe_anneal;
typedef struct tpe_anneal_dbg {
  int32_t row;          /* chosen history row (-1: prior draw)               */
  int32_t reused;       /* 1: taken from the chain, 0: a new pick            */
  int32_t g;            /* rank of a new pick after the clip (-1 otherwise)  */
  int32_t pad_;
  double p0, p1;        /* (mid, half) | (mu, sigma) | (onehot index, shrink);
                           a prior draw: (a, b)                              */
  double variate;       /* the value draw's u in [0, 1) or standard normal z */
} tpe_anneal_dbg;
int tpe_anneal_sample(const double* vals, const uint8_t* active, int64_t ld, int64_t n_cols,
                      int64_t n_rows, const double* loss, const tpe_anneal* recs,
                      const tpe_anneal* host_recs, int n_recs, const double* p,
                      const int32_t* item_off, const int32_t* item_label, int64_t n_items,
                      const int64_t* new_ids, int64_t n_trials, double avg_best_idx,
                      int32_t* chain, int32_t* chain_n, int chain_ld, double* out,
                      tpe_anneal_dbg* dbg, int32_t* err, void* stream);
/* host: writes sizeof(tpe_anneal, tpe_anneal_dbg) to out[0..n); returns 2 */
int tpe_anneal_struct_sizes(int32_t* out, int n);

/* ---- a fixed pool of configurations (tpe.suggest_from_pool) ----------------
 * A pool is n_rows configurations in HBM, label-major like a history: label
 * j's values are one contiguous fp64 column (handed to the exact scorers above
 * as their `cand`, TPE_F_INJECTED) and its activity one byte per row at
 * active + j * ld.  The criterion of a whole configuration is broadcast_best's
 * (tpe.py:649-658) summed over its live labels (build_posterior factorises
 * over labels, tpe.py:697-746):
 *   S[r] = sum_{j active in row r} (below_llik_j[r] - above_llik_j[r]).
 *
 * tpe_pool_fold adds n_labels labels to S, in list order: label i's
 * log-densities are the n_rows elements at bl + host_off[i] / al + host_off[i]
 * (the scorers' out_bl / out_al), its column host_col[i].  init != 0: S starts
 * at 0.0, otherwise at its content (a pool scored in label chunks).  An
 * inactive label is skipped, not added as zero; the sum is sequential fp64 in
 * list order.  terms (nullable): label i's term (NaN where inactive) is also
 * written to terms + host_col[i] * terms_ld.  host_off / host_col: host
 * arrays, read before the call returns. */
int tpe_pool_fold(const double* bl, const double* al, const int64_t* host_off,
                  const int64_t* host_col, int n_labels, const uint8_t* active, int64_t ld,
                  int64_t n_rows, int init, double* S, double* terms, int64_t terms_ld,
                  void* stream);
/* tpe_pool_topk: the first min(k, untaken rows) rows r with taken[r] == 0 in
 * np.argmax order -- larger score first, NaN before everything, equal scores
 * (-0.0 == +0.0) to the smaller row -- written to out_rows in rank order, their
 * number to *out_count (entries of out_rows past it are left alone).  Exact
 * (a multi-block radix select over the score bits, then a ranking of the
 * selected rows); no floating-point atomics, the result does not depend on
 * block scheduling.  scratch: tpe_pool_topk_scratch_bytes(n_rows, k) bytes
 * (-1: bad arguments).
 *
 * tpe_pool_topk_layout (host only, no GPU call): where a call with these
 * (n_rows, k) keeps its intermediate state in `scratch`, which is still there
 * when the call has ended.  Writes up to n of these seven numbers to out and
 * returns how many it wrote (-1: bad arguments): the byte offsets of
 *   [0] the control block, five 64-bit words: prefix (the key T of the last
 *       selected row once the eight passes are done), mask (the key bits
 *       decided so far), k_rem (rows with key == T that are selected), k_eff
 *       (rows selected: min(k, untaken rows)), n_less (selected rows with
 *       key < T); three more words pad it to 64 bytes,
 *   [1] the 256 uint64 radix bins (zero after every pass),
 *   [2] the tile table, two int64 per tile of out[6] rows: the number of
 *       untaken rows with key < T and with key == T in the tiles before it,
 *   [3] cand_key and [4] cand_row, min(k, n_rows) 64-bit slots each: the
 *       selected rows -- those with key < T in row order, then the first k_rem
 *       with key == T -- before they are ranked,
 * then [5] the total, tpe_pool_topk_scratch_bytes(n_rows, k), and [6] the rows
 * per tile.  key = ~order_key(score): ascending key is rank order, every NaN
 * has key 1, -0.0 the key of +0.0. */
int64_t tpe_pool_topk_scratch_bytes(int64_t n_rows, int64_t k);
int tpe_pool_topk_layout(int64_t n_rows, int64_t k, int64_t* out, int n);
int tpe_pool_topk(const double* score, const uint8_t* taken, int64_t n_rows, int64_t k,
                  int64_t* out_rows, int64_t* out_count, void* scratch, void* stream);

/* ---- a pool sampled from the posterior (tpe.Pool.sample) --------------------
 * The scorers' own draws (out_x, candidate r of every label's stream) read as
 * configuration r, in the pool layout above.
 *
 * tpe_rows_active: which labels are live in each row, from the row's own
 * selector values.  The space's liveness is a program in CSR form: label j's
 * clauses are [host_label_off[j], host_label_off[j + 1]), clause c's terms
 * [host_clause_off[c], host_clause_off[c + 1]).  A term holds in row r iff
 * llrint(vals[col * ld + r]) == value (never for a NaN or an infinity), a
 * clause iff all its terms hold (none: always), a label is live iff one of its
 * clauses holds (none: never).  Writes active[j * ld + r] (0 / 1) for r <
 * n_rows and adds label j's live rows to n_active[j] (device, zeroed by the
 * caller; integer adds).  Limits: TPE_COND_MAX_LABELS labels,
 * TPE_COND_MAX_CLAUSES clauses, TPE_COND_MAX_TERMS terms -- a larger program
 * returns TPE_E_UNSUPPORTED.  host_*: host arrays, read before the call
 * returns. */
#define TPE_COND_MAX_LABELS 128
#define TPE_COND_MAX_CLAUSES 256
#define TPE_COND_MAX_TERMS 256
typedef struct tpe_cond_term {
  int32_t col;          /* the selector's column, in [0, n_labels)             */
  int32_t value;        /* the branch index the selector must hold             */
} tpe_cond_term;
int tpe_rows_active(const double* vals, int64_t ld, int64_t n_rows, int n_labels,
                    const int32_t* host_label_off, const int32_t* host_clause_off,
                    const tpe_cond_term* host_terms, int n_terms, uint8_t* active,
                    int64_t* n_active, void* stream);
/* tpe_pool_ranges: out[2 j], out[2 j + 1] (device) = (min, max) of label j's
 * live finite values, with host_positive[j] != 0 of those > 0 only; a label
 * without such a value: (+inf, -inf).  -0.0 orders below +0.0.  Exact and
 * independent of block scheduling (integer min / max of order-preserving
 * keys). */
int tpe_pool_ranges(const double* vals, const uint8_t* active, int64_t ld, int64_t n_rows,
                    int n_labels, const uint8_t* host_positive, double* out, void* stream);
/* tpe_pool_take: rows[0, k) (device, e.g. tpe_pool_topk's out_rows) gathered
 * into out_vals (k, n_labels) fp64 and out_active (k, n_labels) bytes,
 * row-major; a row outside [0, ld) gives NaN / 0. */
int tpe_pool_take(const double* vals, const uint8_t* active, int64_t ld, int n_labels,
                  const int64_t* rows, int64_t k, double* out_vals, uint8_t* out_active,
                  void* stream);
/* host: writes sizeof(tpe_cond_term) to out[0..n); returns 1 */
int tpe_sampled_struct_sizes(int32_t* out, int n);

/* ---- distinct configurations of a pool (tpe.distinct_rows) -------------------
 * Two rows hold the same configuration iff their activity bytes agree for
 * every label and, for every label live in them, their values are equal as
 * fp64 numbers with -0.0 == +0.0 and all NaNs equal (the scorers' order_key);
 * entries of labels that are not live are ignored.
 *
 * tpe_pool_distinct: for the pool rows [0, n_rows) (layout above) and a list
 * of n_seen seen rows -- label-major like the pool, at seen_vals / seen_active
 * with leading dimension seen_ld (a DeviceHistory's vals / active / ld);
 * position t of the list is row seen_rows[t] (device int32; an entry outside
 * [0, seen_ld) is ignored), or row t when seen_rows is NULL --
 *   first[r] = -1 - t, t the smallest position of the list whose row holds
 *              r's configuration, if there is one; otherwise
 *            = the smallest pool row that holds r's configuration.
 * A row is fresh iff first[r] == r.  host_seen_shift (host, per label, or
 * NULL; read before the call returns): subtracted from the seen value of the
 * label before it is compared (a history stores randint(low, high) with `low`
 * included, a pool without); a nonzero entry only among the first
 * TPE_DISTINCT_SHIFT_LABELS labels (else TPE_E_UNSUPPORTED).  mask_out
 * (nullable): mask_out[r] = (taken_in ? taken_in[r] : 0) | (first[r] != r),
 * tpe_pool_topk's `taken`; nothing past n_rows is written.  hash_bits in
 * [0, 64]: the bits of the row hash that are kept -- 64 in the product; fewer
 * put unequal rows on one probe chain (0: all rows on one), which costs time
 * and nothing else.  Exact (rows are equal only after a value-by-value
 * comparison) and independent of block scheduling (integer atomics on an
 * open-addressing table in `scratch`); asynchronous on `stream`, no
 * allocation.  scratch: tpe_pool_distinct_scratch_bytes(n_rows, n_seen) bytes
 * (-1: bad arguments), 8-byte aligned.  n_rows == 0 and n_seen == 0 are
 * legal. */
#define TPE_DISTINCT_SHIFT_LABELS 4096
int64_t tpe_pool_distinct_scratch_bytes(int64_t n_rows, int64_t n_seen);
int tpe_pool_distinct(const double* vals, const uint8_t* active, int64_t ld, int64_t n_rows,
                      int n_labels, const double* seen_vals, const uint8_t* seen_active,
                      int64_t seen_ld, const int32_t* seen_rows, int64_t n_seen,
                      const double* host_seen_shift, int hash_bits, const uint8_t* taken_in,
                      int64_t* first, uint8_t* mask_out, void* scratch, void* stream);

/* ---- a grid pool: the product of per-label axes (tpe.GridPool) ---------------
 * The criterion above is separable: once the scorers have left log l / log g
 * of every axis value in bl / al, the score of a row of the product is a sum
 * of per-value terms.  tpe_grid_fold writes it for one block of a grid -- the
 * product of n_labels axes, row r holding the mixed-radix digits of r, last
 * label fastest (itertools.product order) -- and a window of its rows:
 *   S_out[i] = sum_j (bl[host_off[j] + d_j] - al[host_off[j] + d_j]),
 *   d_j = digit j of row row_begin + i,   i in [0, n_rows),
 * a sequential fp64 sum from 0.0 in list order: the bits tpe_pool_fold gives
 * for the materialised row.  host_off[j]: the element of label j's digit 0;
 * host_radix[j] >= 1 its number of digits (a label fixed in the block: radix 1
 * and an offset that points at its value).  The block has prod host_radix
 * rows, which must fit int64 and hold the window.  Only entries of digits that
 * rows of the window take are read, so an offset may be negative where the
 * caller keeps a slice of an axis's terms.  n_labels <= 128.  host_off /
 * host_radix: host arrays, read before the call returns.  One launch, no
 * atomics; the result does not depend on block scheduling. */
int tpe_grid_fold(const double* bl, const double* al, const int64_t* host_off,
                  const int64_t* host_radix, int n_labels, int64_t row_begin, int64_t n_rows,
                  double* S_out, void* stream);

/* ---- a joint (multivariate) Parzen criterion over a pool's rows --------------
 * (tpe.score_configs(joint=True); the model: hyperopt_amd/joint.py.)  One set
 * -- below or above -- is a mixture of n + 1 product kernels over the D joint
 * labels, one per trial of the set in row order and the prior last:
 *   a_i      = log w_i + sum_d log k_{d,i}(c_d)   (d in list order, from log w_i)
 *   log L(c) = m + log sum_i exp(a_i - m),  m = max_i a_i   (-inf when m is).
 * A label's factor, with t(x) = log(max(x, 1e-12)) for TPE_JOINT_LOG and x
 * otherwise, sigma the set's bandwidth for a trial component and prior_sigma
 * for the prior, Phi the device's normal_cdf and Z = Phi(hi) - Phi(lo) for
 * TPE_JOINT_BOUNDED (else 1):
 *   TPE_JOINT_CONT   -u^2 - log(sigma sqrt(2 pi)) - log Z,
 *                    u = (t(x) - mu) * (1 / (sqrt(2) sigma))
 *   TPE_JOINT_QUANT  log(Phi(t(x + q/2)) - Phi(t(x - q/2))) - log Z, the edges
 *                    clipped to [lo, hi] when bounded; otherwise a lower edge
 *                    <= 0 of a log label gives Phi = 0; a mass <= 0: -inf
 *   TPE_JOINT_CAT    tables[tab_off + x] where x equals the component's
 *                    category, tables[tab_off + n_cat + x] where not, and
 *                    tables[tab_off + 2 n_cat + x] for the prior component.
 *
 * A prepared set is tpe_joint_set_doubles(D, n) doubles on the device (-1: bad
 * arguments), 16-byte aligned.  The caller writes its head: log w (n + 1),
 * then the D bandwidths sigma, then the D values 1 / (sqrt(2) sigma).
 * tpe_joint_prep writes the rest from a label-major history (hist_vals /
 * hist_active, leading dimension hist_ld, hist_cols columns; a DeviceHistory's):
 * component i < n is history row rows[i] (device int32), or row i when rows
 * is NULL; per label its mu -- t(value - shift), the category for a discrete
 * label -- and the constant of the factor above.  The labels are given twice:
 * host_labels is read before the call returns (checks), labels is the same
 * array on the device.
 *
 * tpe_joint_score: out[i] = log L(row row_begin + i) - (sub ? sub[i] : 0) for
 * i in [0, n_rows), rows of a label-major pool (vals, ld, n_cols columns; label
 * d's column is labels[d].col).  The components are scored in chunks of
 * TPE_JOINT_CHUNK (one partial (m, s) per row and chunk in `scratch`,
 * tpe_joint_scratch_bytes(n_rows, n) bytes, 16-byte aligned) and merged in
 * chunk order.  A row's bits depend on the row, the set and that constant
 * alone: not on the grid, the row window or block scheduling; no
 * floating-point atomics.  Limits: D <= TPE_COND_MAX_LABELS, n_cat <=
 * TPE_JOINT_MAX_CAT, else TPE_E_UNSUPPORTED; bad arguments return TPE_E_ARG
 * before any launch.  Asynchronous on `stream`, no allocation. */
#define TPE_JOINT_CHUNK 256
#define TPE_JOINT_MAX_CAT 65536
enum { TPE_JOINT_CONT = 0, TPE_JOINT_QUANT = 1, TPE_JOINT_CAT = 2 };
enum { TPE_JOINT_LOG = 1, TPE_JOINT_BOUNDED = 2 };
typedef struct tpe_joint_label {
  int32_t kind;         /* TPE_JOINT_CONT / QUANT / CAT                        */
  int32_t flags;        /* TPE_JOINT_LOG | TPE_JOINT_BOUNDED                   */
  int32_t col;          /* the label's column in the pool and in the history   */
  int32_t n_cat;        /* CAT: number of options                              */
  double lo, hi;        /* BOUNDED: the bounds in the fit coordinate           */
  double q;             /* QUANT: the step                                     */
  double prior_mu, prior_sigma;
  double prior_r;       /* 1 / (sqrt(2) prior_sigma)                           */
  double shift;         /* subtracted from a history value (randint's low)     */
  int64_t tab_off;      /* CAT: its 3 n_cat entries of `tables`                */
} tpe_joint_label;
int64_t tpe_joint_set_doubles(int n_labels, int64_t n);
int64_t tpe_joint_scratch_bytes(int64_t n_rows, int64_t n);
int tpe_joint_prep(const tpe_joint_label* host_labels, const tpe_joint_label* labels,
                   int n_labels, const double* hist_vals, const uint8_t* hist_active,
                   int64_t hist_ld, int hist_cols, const int32_t* rows, int64_t n, double* set,
                   void* stream);
int tpe_joint_score(const tpe_joint_label* host_labels, const tpe_joint_label* labels,
                    int n_labels, const double* tables, int64_t n_tables, const double* set,
                    int64_t n, const double* vals, int64_t ld, int n_cols, int64_t row_begin,
                    int64_t n_rows, const double* sub, double* out, void* scratch, void* stream);
/* host: TPE_JOINT_CHUNK as the library was built */
int tpe_joint_chunk(void);
/* host: writes sizeof(tpe_joint_label) to out[0..n); returns 1 */
int tpe_joint_struct_sizes(int32_t* out, int n);

/* ---- the joint criterion on a block of a grid pool (tpe.GridPool(joint=True)) -
 * In tpe_joint_score's sum every joint label d adds to a_i a factor that
 * depends on the label, the component and the label's value alone.  On a grid
 * that value is one of the axis's values, so a set's factors form a table F of
 * (sum of the axis lengths) x C doubles, and a row's a_i is log w_i plus one
 * entry per joint label, added in label order: the same sequence of roundings.
 * The results have the bits tpe_joint_score gives the materialised rows under
 * the same prepared set.
 *
 * Components go in windows [comp_begin, comp_begin + n_comp): comp_begin and
 * n_comp multiples of TPE_JOINT_CHUNK, comp_begin <= n, n_comp <= ldF, ldF
 * even (places past the set's last component are padding).
 *
 * tpe_grid_joint_factors: for label d of a prepared set's n_labels labels and
 * every value v of its axis -- axes[host_axis_off[d] + v], v in [0,
 * host_axis_len[d]), stored values as a pool holds them -- and every component
 * i of the window, F[(host_frow[d] + v) * ldF + (i - comp_begin)] = the factor
 * of tpe_joint_score's sum (0.0 past the last component).  n_axes: the doubles
 * of `axes`; n_frows: the rows of F.  One launch per label.
 *
 * tpe_grid_joint_score: rows [row_begin, row_begin + n_rows) of one block of a
 * grid (tpe_grid_fold's decode: n_labels labels of host_radix[j] >= 1 digits,
 * the last fastest).  host_frow[j] is the F row of label j's digit 0, or < 0
 * for a label that only takes part in the decode; the joint labels add their
 * entries in list order.  Each call scores one component window into
 * `scratch` (tpe_grid_joint_scratch_bytes(n_rows, n) bytes, 16-byte aligned,
 * kept by the caller from the set's first window to its last, every window
 * given once).  `last` says that the window holds the set's last component
 * (checked); that call also merges the row's chunks in chunk order:
 *   v = log L(row row_begin + i) - (sub ? sub[i] : 0)
 *   TPE_GRID_JOINT_STORE   out[i] = v
 *   TPE_GRID_JOINT_ADD     out[i] = out[i] + v
 * Limits: n_labels <= 128 (else TPE_E_UNSUPPORTED), n_frows < 2^31; bad
 * arguments return TPE_E_ARG before any launch.  Asynchronous on `stream`, no
 * allocation, no atomics; a row's bits do not depend on the windows.
 *
 * tpe_grid_joint_layout (host): out[0..n) <- the rows of a tile, the chunk,
 * the components per pass, the label limit; returns the count written.
 *
 * tpe_grid_fold_onto: tpe_grid_fold, except that the sum starts from S[i] as
 * it stands (S[i] = S[i] + term_0 + ...), and that a label with host_off[j] < 0
 * is decoded but adds nothing. */
enum { TPE_GRID_JOINT_STORE = 0, TPE_GRID_JOINT_ADD = 1 };
int tpe_grid_joint_layout(int64_t* out, int n);
int64_t tpe_grid_joint_scratch_bytes(int64_t n_rows, int64_t n);
int tpe_grid_joint_factors(const tpe_joint_label* host_labels, const tpe_joint_label* labels,
                           int n_labels, const double* tables, int64_t n_tables,
                           const double* set, int64_t n, const double* axes, int64_t n_axes,
                           const int64_t* host_axis_off, const int64_t* host_axis_len,
                           const int64_t* host_frow, double* F, int64_t ldF, int64_t n_frows,
                           int64_t comp_begin, int64_t n_comp, void* stream);
int tpe_grid_joint_score(const double* F, int64_t ldF, int64_t n_frows, int64_t comp_begin,
                         int64_t n_comp, const double* set, int64_t n, const int64_t* host_radix,
                         const int64_t* host_frow, int n_labels, int64_t row_begin,
                         int64_t n_rows, const double* sub, double* out, int out_mode,
                         void* scratch, int last, void* stream);
int tpe_grid_fold_onto(const double* bl, const double* al, const int64_t* host_off,
                       const int64_t* host_radix, int n_labels, int64_t row_begin, int64_t n_rows,
                       double* S, void* stream);

/* ---- rows drawn from a set's joint mixture (tpe.Pool.sample(joint=True)) -----
 * tpe_joint_sample: row g = row_base + r, r in [0, n_rows), is one draw from the
 * mixture of a prepared set (above: n trial components in row order, the prior
 * last), written to vals[labels[d].col * ld + r] for every label d -- a
 * label-major block of n_cols columns whose row 0 is row row_base.  Philox
 * counters are {g lo, g hi, attempt, 0x4A4F494E "JOIN"}; keys (device) holds
 * the D label keys, then the component key.
 *   component   key keys[D], call (g, 0): word x picks the first i with
 *               cdf[i] > x 2^-32 cdf[n] -- cdf: n + 1 doubles on the device, the
 *               running sum of the components' weights, the prior's last.
 *   TPE_JOINT_CONT / QUANT   key keys[d], attempts a = 0, 1, ... at (g, a):
 *               t = mu + sigma z, z the Box-Muller normal of words y, z, w;
 *               (mu, sigma) the component's (the set's mu and bandwidth of
 *               label d, or prior_mu / prior_sigma).  TPE_JOINT_BOUNDED accepts
 *               lo <= t < hi; after 256 rejections the last t is clamped to lo
 *               or to nextafter(hi, -inf).  x = exp(t) for TPE_JOINT_LOG, else
 *               t; QUANT stores rint(x / q) q.
 *   TPE_JOINT_CAT   key keys[d], call (g, 0).  The label's cdf is the n_cat
 *               doubles at cat_cdf[tab_off / 3] (device; n_cat_cdf doubles in
 *               all: one n_cat-entry running sum of the prior probabilities
 *               per discrete label, packed in the order of `tables`, so tab_off
 *               is a multiple of 3).  A trial component of category c keeps c
 *               when x 2^-32 one_plus_a < 1 (one_plus_a = 1 + cat_smoothing
 *               >= 1) and otherwise draws with word y; the prior component
 *               draws with word x.  A word picks the first k with word <
 *               ceil(cdf[k] / cdf[n_cat - 1] 2^32) (saturated at 2^32 - 1; the
 *               word 2^32 - 1 is read as 2^32 - 2), the last k if none.  The
 *               stored value is the category index.
 * comp_out (device, nullable): comp_out[r] = the row's component, n for the
 * prior.  One thread per (row, label), 256 rows per block; the cdf is staged
 * in LDS up to TPE_JOINT_SAMPLE_STAGE components and searched in global memory
 * above.  A row's values depend on (keys, g, the set, the labels) alone: not on
 * the grid, the row window or block scheduling; no atomics.  Limits as above
 * (TPE_E_UNSUPPORTED); n < 2^31 - 1, n_rows <= ld; bad arguments return
 * TPE_E_ARG before any launch; n_rows == 0 is a no-op.  Asynchronous on
 * `stream`, no allocation. */
#define TPE_JOINT_SAMPLE_STAGE 64
int tpe_joint_sample(const tpe_joint_label* host_labels, const tpe_joint_label* labels,
                     int n_labels, const double* set, int64_t n, const double* cdf,
                     const double* cat_cdf, int64_t n_cat_cdf, const uint64_t* keys,
                     double one_plus_a, int64_t row_base, int64_t n_rows, double* vals,
                     int64_t ld, int n_cols, int32_t* comp_out, void* stream);
/* host: TPE_JOINT_SAMPLE_STAGE as the library was built */
int tpe_joint_sample_stage(void);

/* ---- the joint criterion on a list of rows (tpe.score_configs(joint="tree")) --
 * A group of labels under a `switch` is live in some pool rows only; its
 * mixture is scored on those (hyperopt_amd/joint.py, "Groups").
 *
 * tpe_rows_compact: out_rows[0, c) (device int64) = the ascending indices
 * r < n_rows with flags[r] != 0, *out_count (device int64) = c; entries of
 * out_rows at or past c are not written.  flags: n_rows bytes on the device --
 * one label's row of a pool's label-major `active` block.  Exact and
 * independent of block scheduling: a count per block of rows, an integer scan
 * of the counts, a scatter by the row's rank within its block; no atomics.
 * scratch: tpe_rows_compact_scratch_bytes(n_rows) bytes (-1: bad arguments),
 * 8-byte aligned.  n_rows == 0 writes the count 0 and needs neither flags nor
 * out_rows.  tpe_rows_compact_layout (host): out[0] = the rows one block
 * handles, out[1] = the rows one pass of the scan's single block covers;
 * returns 2.
 *
 * tpe_joint_score_rows: tpe_joint_score (above) with the dense row window
 * replaced by a window of a device list.  List position p in [list_begin,
 * min(list_begin + max_rows, *d_count)) scores pool row rows[p]:
 *   v = log L(row rows[p]) - (sub ? sub[p - list_begin] : 0)
 *   out_mode 0                                       out[p - list_begin] = v
 *   TPE_JOINT_OUT_SCATTER                            out[rows[p]] = v
 *   TPE_JOINT_OUT_SCATTER | TPE_JOINT_OUT_ADD        out[rows[p]] = out[rows[p]] + v
 * (any other out_mode: TPE_E_ARG).  rows (device int64) holds at least
 * *d_count entries; d_count is read on the device only -- the host never
 * learns it, and max_rows, the host's bound, sizes the grid and the scratch
 * (tpe_joint_scratch_bytes(max_rows, n) bytes, 16-byte aligned).  Positions at
 * or past the count write nothing, and a block of 256 positions that starts
 * there returns at once.  An entry outside [0, ld) is skipped: nothing of that
 * row is read and nothing is written for it (a device list cannot be checked
 * by the host, and a bad one must not fault).  A list holds distinct rows:
 * with a row listed twice the scattering modes write it twice, in no stated
 * order.  out: max_rows doubles for out_mode 0, ld doubles otherwise.  log L of
 * a row has the bits tpe_joint_score gives that row under the same prepared
 * set.  Limits, errors and stream conventions as tpe_joint_score; max_rows ==
 * 0 and ld == 0 are no-ops. */
enum { TPE_JOINT_OUT_SCATTER = 1, TPE_JOINT_OUT_ADD = 2 };
int64_t tpe_rows_compact_scratch_bytes(int64_t n_rows);
int tpe_rows_compact_layout(int64_t* out, int n);
int tpe_rows_compact(const uint8_t* flags, int64_t n_rows, int64_t* out_rows, int64_t* out_count,
                     void* scratch, void* stream);
int tpe_joint_score_rows(const tpe_joint_label* host_labels, const tpe_joint_label* labels,
                         int n_labels, const double* tables, int64_t n_tables, const double* set,
                         int64_t n, const double* vals, int64_t ld, int n_cols,
                         const int64_t* rows, const int64_t* d_count, int64_t list_begin,
                         int64_t max_rows, const double* sub, double* out, int out_mode,
                         void* scratch, void* stream);

/* ---- a group's mixture conditioned on its context -----------------------------
 * (tpe.score_configs(joint="chain"); hyperopt_amd/joint.py, "Chains".)
 * tpe_joint_chain_rows: tpe_joint_score_rows on a set prepared over the labels
 * ctx + g, the n_ctx context labels first, with
 *   v = (log L(row) - log L_ctx(row)) - (sub ? sub[p - list_begin] : 0)
 * log L_ctx: the same mixture with the factors of labels [n_ctx, n_labels)
 * dropped -- a_i cut off after the first n_ctx labels, the same components,
 * weights and sigmas.  Both come from one walk over the labels; log L has the
 * bits tpe_joint_score_rows gives the row under this set, log L_ctx the bits it
 * gives with n_labels = n_ctx under a set prepared from the first n_ctx labels
 * with this set's sigmas.  -inf - -inf is NaN and is written.  n_ctx <= 0 or
 * n_ctx >= n_labels: TPE_E_ARG.  scratch: tpe_joint_chain_scratch_bytes(
 * max_rows, n) bytes (-1: bad arguments), 16-byte aligned.  Everything else --
 * the list, the three out_modes, skipped entries, limits, errors, no-ops -- as
 * tpe_joint_score_rows. */
int64_t tpe_joint_chain_scratch_bytes(int64_t n_rows, int64_t n);
int tpe_joint_chain_rows(const tpe_joint_label* host_labels, const tpe_joint_label* labels,
                         int n_labels, int n_ctx, const double* tables, int64_t n_tables,
                         const double* set, int64_t n, const double* vals, int64_t ld, int n_cols,
                         const int64_t* rows, const int64_t* d_count, int64_t list_begin,
                         int64_t max_rows, const double* sub, double* out, int out_mode,
                         void* scratch, void* stream);

/* ---- a batch picked one at a time under the joint criterion -------------------
 * (tpe.suggest_from_pool(joint=True, batch="liar"); hyperopt_amd/joint.py,
 * "Batches".)  Pick j enters the above mixture as one more trial component
 * whose observation is its own row p of the pool -- mu and the constant as
 * tpe_joint_prep forms them, the factors as tpe_joint_score's -- of weight
 * exp(log_lie):
 *   c_p(r) = log_lie + sum_d log k_d(r_d)              (d in list order)
 *   U_0[r] = log_w + A0[r]
 *   U_j[r] = m + log(exp(U_{j-1}[r] - m) + exp(c_p(r) - m)), m = max of the two
 *            (c_p(r) = -inf leaves U's bits; m = -inf gives -inf)
 *   S_j[r] = S0[r] - (U_j[r] - U_0[r]) where U_0[r] is finite, else S0[r].
 * Pick j + 1 is the first row of S_j in tpe_pool_topk's order (larger first, NaN
 * before everything, equal scores to the smaller row) among the rows r with
 * taken[r] == 0, (distinct ? distinct[r] == 0 : true) and not picked before;
 * the run stops when no row is left.
 *
 * labels / tables as tpe_joint_score takes them.  sigma (device): the above
 * set's D bandwidths, then the D values 1 / (sqrt(2) sigma) -- a prepared set's
 * head from element n + 1 on (may be NULL when every label is discrete).
 * vals, ld, n_cols: the label-major pool, rows [0, n_rows).  S0, A0 (n_rows
 * doubles), taken and distinct (n_rows bytes; distinct may be NULL) are read
 * only.  out_rows: k device int64, entries [0, *out_count) written in pick
 * order; out_count: device int64.  S_at_pick (k doubles, optional): entry j =
 * S_j of pick j + 1, the score it was picked at.  S_k (n_rows doubles,
 * optional): the score after the last pick made.  scratch:
 * tpe_joint_lie_scratch_bytes(n_rows) bytes (-1: bad arguments), 16-byte
 * aligned; it holds the working copies.  k > n_rows counts as n_rows.
 *
 * All picks are enqueued by the one call: a pick's row is read on the device,
 * the host learns nothing before it reads out_count / out_rows.  A row's bits
 * depend on the row, the labels and the pick sequence only -- not on n_rows,
 * the block a row falls in or block scheduling; no floating-point atomics.
 * Limits as tpe_joint_score (TPE_E_UNSUPPORTED); bad arguments return TPE_E_ARG
 * before any launch; k <= 0 or n_rows == 0 writes the count 0 (and S0 to S_k
 * where given).  Asynchronous on `stream`, no allocation. */
int64_t tpe_joint_lie_scratch_bytes(int64_t n_rows);
int tpe_joint_lie_picks(const tpe_joint_label* host_labels, const tpe_joint_label* labels,
                        int n_labels, const double* tables, int64_t n_tables,
                        const double* sigma, const double* vals, int64_t ld, int n_cols,
                        int64_t n_rows, const double* S0, const double* A0, double log_w,
                        double log_lie, const uint8_t* taken, const uint8_t* distinct,
                        int64_t k, int64_t* out_rows, int64_t* out_count, double* S_at_pick,
                        double* S_k, void* scratch, void* stream);

/* ---- argmax combine: n_sets tpe_best arrays of n_labels each (e.g. one per
 * rank after an all-gather) -> n_labels winners, same tie rules. ------------ */
int tpe_best_combine(const tpe_best* sets, int n_sets, int n_labels, tpe_best* out,
                     void* stream);

/* ---- per-label records of one rank's level: slot s of `out` (n_slots
 * tpe_best, device) <- the records of the jobs j with slot[j] == s (device
 * int32 per job), folded in job order with the argmax rules; index -1 where
 * no job maps to s.  The input of tpe_maxloc_allreduce for a label-sharded
 * level. */
int tpe_best_scatter(const tpe_best* by_job, const int32_t* slot, int n_jobs, tpe_best* out,
                     int n_slots, void* stream);

/* ---- cross-GPU max-loc (replaces the argmax of tpe.py:650-658
 * across ranks): all-gather of every rank's n_labels records over the caller's
 * RCCL communicator `comm` (an ncclComm_t; librccl.so.1 is bound at the first
 * call), then tpe_best_combine of the world's sets into `out`.  `local`: this
 * rank's records (index -1 where it scored nothing); `gathered`: device
 * scratch of world * n_labels records.  Asynchronous on `stream`. */
int tpe_maxloc_allreduce(const tpe_best* local, tpe_best* gathered, tpe_best* out, int n_labels,
                         void* comm, void* stream);

/* ---- level launcher: a whole suggest level's stream work in one host call.
 * `ops` (host) is a list of records, each naming one of the entry points above
 * (or a runtime step) by `code` and carrying that call's arguments, in
 * declaration order, as 64-bit words (pointers and handles as addresses,
 * int / int64_t by value).  tpe_run_ops issues them in order and stops at the
 * first failing record (its index in *failed_op, -1 when all succeeded).  A
 * binding that replays the same level (same kernels, grids, workspace) keeps
 * its record array and re-issues it with one call: the per-call inputs live
 * in the device buffers the records point to (the level's upload), or captures
 * them once into a hipGraph and replays that (tpe_ops_capture below). ------ */
enum {
  TPE_OP_GATHER_OBS = 1,       /* tpe_gather_obs                             */
  TPE_OP_GATHER_OBS_MULTI,     /* tpe_gather_obs_multi                       */
  TPE_OP_PARZEN_FIT,           /* tpe_parzen_fit                             */
  TPE_OP_CAT_POSTERIOR,        /* tpe_cat_posterior                          */
  TPE_OP_TABLE_BUILD,          /* tpe_table_build                            */
  TPE_OP_SCORE_TABLE,          /* tpe_score_table                            */
  TPE_OP_SCORE_TABLE_FAST,     /* tpe_score_table_fast                       */
  TPE_OP_SCORE_PRUNED64,       /* tpe_score_pruned64                         */
  TPE_OP_SCORE_CONTINUOUS,     /* tpe_score_continuous                       */
  TPE_OP_SORT_CANDIDATES,      /* tpe_sort_candidates                        */
  TPE_OP_SCORE_SORTED,         /* tpe_score_sorted                           */
  TPE_OP_LATTICE_SAMPLE,       /* tpe_lattice_sample                         */
  TPE_OP_LATTICE_COMPACT,      /* tpe_lattice_compact                        */
  TPE_OP_SCORE_QUANTIZED,      /* tpe_score_quantized                        */
  TPE_OP_SCORE_CATEGORICAL,    /* tpe_score_categorical                      */
  TPE_OP_SAMPLE,               /* tpe_sample                                 */
  TPE_OP_EVENT_RECORD,         /* hipEventRecord(a[0] event, a[1] stream)    */
  TPE_OP_STREAM_WAIT,          /* hipStreamWaitEvent(a[0] stream, a[1] event) */
  TPE_OP_MEMCPY,               /* hipMemcpyAsync(a[0] dst, a[1] src, a[2] bytes,
                                  a[3] hipMemcpyKind, a[4] stream)           */
  TPE_OP_STREAM_SYNC,          /* hipStreamSynchronize(a[0] stream)          */
  TPE_OP_BEST_SCATTER,         /* tpe_best_scatter                           */
  TPE_OP_MAXLOC_ALLREDUCE,     /* tpe_maxloc_allreduce (RCCL, stream-ordered) */
  TPE_OP_LATTICE_SUGGEST,      /* tpe_lattice_suggest                        */
  TPE_OP_BAND_RESCORE,         /* tpe_band_rescore                           */
  TPE_OP_FIT_SORTED,           /* tpe_fit_sorted                             */
  TPE_OP_HISTORY_ORDER,        /* tpe_history_order                          */
  TPE_OP_CATEGORICAL_SUGGEST,  /* tpe_categorical_suggest                    */
  TPE_OP_CAT_POSTERIOR_HIST,   /* tpe_cat_posterior_hist                     */
  TPE_OP_COUNT
};
#define TPE_OP_ARGS 23
typedef struct tpe_op {
  int32_t code;
  int32_t n_args;               /* must equal the entry point's parameter count */
  int64_t a[TPE_OP_ARGS];
} tpe_op;                       /* 192 bytes */
int tpe_run_ops(const tpe_op* ops, int n_ops, int* failed_op);
/* Issuing threads of tpe_run_ops (1, the default, or 2); returns the previous
 * setting, TPE_E_ARG for another n.  With 2, a batch whose records use more
 * than one stream is issued by the caller (the records on the stream of the
 * first record that names one, and records without a stream) and a resident
 * worker thread of the library (every other stream's records), each in list
 * order; event records (TPE_OP_EVENT_RECORD / TPE_OP_STREAM_WAIT) are issued
 * in their global list order, so the streams' work and dependencies are those
 * of one-thread issue.  *failed_op names the first failing record in list
 * order.  A batch issued while another thread's batch holds the worker is
 * issued by the caller alone. */
int tpe_set_issue_threads(int n);
/* The same records as a hipGraph: tpe_ops_capture issues ops[0..n_ops) into a
 * stream capture of `capture_stream` (a stream of the caller's, not the null
 * stream), with every record's stream operand that names `from_stream` (the
 * records' main stream, possibly the null stream) pointed at
 * `capture_stream` instead; every stream the records fork to must be joined
 * back by an event wait among the records.  The graph is instantiated in
 * *graph_exec -- nothing runs.  Records that cannot be captured
 * (TPE_OP_STREAM_SYNC, TPE_OP_MAXLOC_ALLREDUCE) fail it with TPE_E_ARG at
 * *failed_op; a capture the runtime refuses fails it with TPE_E_LAUNCH.  The
 * graph holds every record's words as captured (pointers, sizes, grids): a
 * binding replays it with tpe_graph_launch only while re-issuing exactly those
 * records, the per-call inputs again in the device buffers they point to.
 * tpe_graph_destroy frees it. */
int tpe_ops_capture(const tpe_op* ops, int n_ops, void* from_stream, void* capture_stream,
                    void** graph_exec, int* failed_op);
int tpe_graph_launch(void* graph_exec, void* stream);
int tpe_graph_destroy(void* graph_exec);

/* host: rows of the k smallest losses in np.argsort(losses, kind="stable")
 * order (NaN after +inf, ties to the earlier row) -- the below split of
 * ap_split_trials (tpe.py:623-646) -- written to out (host) in ascending row
 * order; returns min(k, n), -1 on bad arguments. */
int64_t tpe_smallest_rows(const double* losses, int64_t n, int64_t k, int64_t* out);
/* host: tpe_smallest_rows plus the level inputs of the split in one pass:
 * isb[r] = 1 for the below rows (else 0), nb[j] = active below rows of label
 * j, na[j] = n_active[j] - nb[j] (a history without from_tid aliasing: every
 * row is below or above).  active: T x L bytes, row-major.  Returns the
 * number of below rows written to below_rows (ascending), -1 on bad
 * arguments (ap_split_trials, tpe.py:623-646). */
int64_t tpe_split_inputs(const double* losses, int64_t T, int64_t n_below, const uint8_t* active,
                         int64_t L, const int64_t* n_active, uint8_t* isb, int64_t* below_rows,
                         int64_t* nb, int64_t* na);

const char* tpe_last_error(void);
int tpe_abi_version(void);
/* Self-check of the hardware transcendentals the fp32 error bounds assume
 * (DESIGN.md 3.1): out[0] = max relative error of v_exp_f32 over every fp32
 * x in [-126, 12]; out[1] = max over positive normal fp32 p of
 * |v_log_f32(p) - log2 p| / max(1, |log2 p|).  Exhaustive (2^32 inputs, a
 * few ms); out: 2 doubles (device), asynchronous on `stream`. */
int tpe_check_transcendentals(double* out, void* stream);
/* Self-check of the categorical counts' exact fold (np.bincount's sequential
 * fp64 sum): one launch folds list[0, n) (device) into s0 in
 * order and writes the sum to out[0] (device), asynchronous on `stream`.
 * scope 0: one wave (the driver of tpe_cat_posterior and of the single-block
 * history count); scope 1: one block (the driver of the chunked history
 * count).  The chain is treated as if `done` entries had been folded before:
 * the first 4096 entries of a chain are added serially, so done >= 4096 skips
 * that prefix and done = 4000 ends it 96 entries into the list.
 * Precondition: every entry and s0 finite and >= 0.  The result must equal
 * the serial chain s = s + w bit for bit. */
int tpe_fold_check(const double* list, int64_t n, double s0, int64_t done, int scope, double* out,
                   void* stream);
/* Self-check of the pruned exact fp64 scorer's exp (exp_neg64, tpe_pruned64.hip):
 * out[i] = exp_neg64(v[i]) for i in [0, n), v and out device arrays,
 * asynchronous on `stream`.  exp_neg64 is specified for v <= 0 and NaN: 0
 * below -745.2, NaN for NaN, else exp(v) within 3.25 * 2^-53 relative (plus
 * 2^-1074 absolute where the result is subnormal). */
int tpe_exp_neg64_check(const double* v, int64_t n, double* out, void* stream);

/* host: writes sizeof(tpe_seg, tpe_cat_seg, tpe_job, tpe_best, tpe_table, tpe_gather,
 * tpe_history, tpe_prior, tpe_op, tpe_band, tpe_colspec) to out[0..n); returns 11 */
int tpe_struct_sizes(int32_t* out, int n);

#ifdef __cplusplus
}
#endif
#endif /* TPE_HIP_H */
