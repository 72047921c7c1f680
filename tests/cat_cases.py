"""Case table shared by tests/test_cat_cases.py (the oracle and the numpy
replay of the streams alone, no GPU) and tests/test_gpu_categorical.py (the
categorical chain on the device: the counts, k_cat_finalize, k_score_cat<4|8|16>
and k_cat_decide of csrc/tpe_fit.hip and csrc/tpe_categorical.hip).

  posterior   randint(K) and categorical(Dirichlet prior) histories of
              max(3 K, 3000) above observations for the K of POSTERIOR_K: below,
              at and above np_pw_leaf's 8 and 128 elements, inside the recursion
              of np_pairwise_sum, and on both sides of numpy's 8192-element
              reduction buffer.  pw_leaf / pairwise / chunked / sequential
              restate the candidate totals; DISCRIMINATING_K are the K at which
              a total formed by the leaf alone, or sequentially, changes bits of
              the above posterior under every setting (elsewhere a wrong total
              may round to the same double: whether a K past 128 tells a broken
              recursion from a working one depends on the history, so the
              premise is asserted, not assumed); at CHUNK_K np.sum differs from
              the pairwise sum of the whole array
  LEVELS      launches of several randint jobs with different K: launch_cat picks
              k_score_cat<KR> from the launch's largest K, so a small K runs
              under every instantiation, and one launch holds all three sampler
              regimes (thresholds in registers, binary search, plain argmax)
  tie         randint(8) whose categories 0 and 5 are observed on neither side:
              bit-equal posteriors, bit-equal scores, the maximum; each of
              below mass 1/33
  zero        categorical(0.3, 0, 0.3, 0, 0.4, 0): category 1 scores NaN (0 / 0),
              category 5 -inf, category 3 +inf
  rare tie    categorical with two categories of the same tiny prior p and no
              observation: tied best scores of below mass ~2e-4, so a prefix of
              4096 candidates holds neither, one or both of them

replay_* give one job's expected outcome in plain numpy: the stream
(oracle.streams.categorical_draw on a cumulative p), the scores (log p_below -
log p_above of the oracle's posteriors), np.argmax's winner, and the `need`
flag of the prefix-first decision.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import streams as S
from oracle import tpe_oracle as O

# the kernels' constants (csrc/tpe_categorical.hip, tpe_fit.hip; no export)
TILE = 4096            # kBS * kRC: candidates of one k_score_cat block
PREFIX = TILE          # the smallest prefix tpe_categorical_suggest accepts
K_KEY = 256            # kCatKey: categories of the rank-key path
KR = (4, 8, 16)        # launch_cat's instantiations
LEAF = 128             # np_pairwise_sum recurses above it
NP_BUF = 8192          # numpy's reduction buffer, in doubles

Job = namedtuple("Job", "name kind args below above key n_cand cand_base")


def _key(i):
    return (0xCA7E60000000000 + 0x9E3779B97F4A7C15 * (i + 1)) & 0xFFFFFFFFFFFFFFFF


# ---------------------------------------------------------------------------
# the totals np.sum could be mistaken for
# ---------------------------------------------------------------------------
def pw_leaf(a):
    """np_pw_leaf: sequential below 8 elements, else 8 accumulators."""
    a = [float(x) for x in a]
    n = len(a)
    if n < 8:
        r = 0.0
        for x in a:
            r += x
        return r
    r = a[:8]
    i = 8
    while i < n - n % 8:
        for j in range(8):
            r[j] += a[i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    while i < n:
        res += a[i]
        i += 1
    return res


def pairwise(a):
    """np_pairwise_sum: numpy's pairwise sum of one buffer."""
    n = len(a)
    if n <= LEAF:
        return pw_leaf(a)
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise(a[:n2]) + pairwise(a[n2:])


def chunked(a):
    """np.sum of a contiguous array: the pairwise sums of the consecutive
    NP_BUF-element chunks, added in order."""
    total = pairwise(a[:NP_BUF])
    for s in range(NP_BUF, len(a), NP_BUF):
        total += pairwise(a[s:s + NP_BUF])
    return total


def sequential(a):
    r = 0.0
    for x in a:
        r += float(x)
    return r


def bits_changed(pseudo, total):
    """Entries of pseudo / total that differ from pseudo / np.sum(pseudo)."""
    return int(np.sum(pseudo / total != pseudo / np.sum(pseudo)))


# ---------------------------------------------------------------------------
# a. posteriors by K
# ---------------------------------------------------------------------------
POSTERIOR_K = (1, 7, 8, 9, 127, 128, 129, 136, 200, 300, 1000, 4097, 8192, 8193, 10000)
DISCRIMINATING_K = (200, 300, 1000)
CHUNK_K = 10000          # np.sum differs from the whole-array pairwise sum here
HIST_K = (33, 129, 200, 300, 1000)    # past kCathMaxCat = 32: the single-block history counts
# (LF, prior weight): the defaults, and one pair of settings_cases' COUNT_LF x COUNT_PW
SETTINGS = ((25, 1.0), (7, 0.3))
KINDS = ("randint", "categorical")
N_BELOW = 25
# history seeds (default: K) moved until the above posterior of every setting
# discriminates at DISCRIMINATING_K (tests/test_cat_cases.py asserts it)
POSTERIOR_SEEDS = {(200, "randint"): 2, (1000, "randint"): 10, (1000, "categorical"): 4}


def n_above(K):
    return max(3 * K, 3000)


@functools.lru_cache(maxsize=None)
def posterior_case(K, kind):
    """(args, below, above) of the posterior history of K categories."""
    rng = np.random.RandomState(POSTERIOR_SEEDS.get((K, kind), K))
    if kind == "randint":
        return (K,), rng.randint(0, K, N_BELOW), rng.randint(0, K, n_above(K))
    p = rng.dirichlet(np.full(K, 0.5))
    return (tuple(p.tolist()),), rng.choice(K, size=N_BELOW, p=p), \
        rng.choice(K, size=n_above(K), p=p)


def pseudocounts(kind, args, obs, pw, lf):
    """The array whose np.sum normalises the posterior (tpe.py:578-615)."""
    obs = np.asarray(obs, np.int64)
    if kind == "randint":
        K = int(args[0])
        return np.bincount(obs, O.linear_forgetting_weights(obs.size, lf), K) + pw
    p = np.asarray(args[0], np.float64)
    return np.bincount(obs, O.linear_forgetting_weights(obs.size, lf), p.size) + \
        p.size * (pw * p)


def posterior(kind, args, obs, pw=1.0, lf=O.DEFAULT_LF):
    if kind == "randint":
        return O.randint_posterior(obs, pw, int(args[0]), lf=lf)
    return O.categorical_posterior(obs, pw, args[0], lf)


@functools.lru_cache(maxsize=None)
def history_case(K):
    """(mat, active, is_below, prior p) of the resident-history case: column 0
    the categorical label, column 1 randint(2, 2 + K) stored with its low."""
    T = n_above(K) + N_BELOW
    rng = np.random.RandomState(5000 + K)
    p = rng.dirichlet(np.full(K, 0.5))
    mat = np.stack([rng.choice(K, size=T, p=p).astype(float),
                    (rng.randint(0, K, T) + 2).astype(float)], axis=1)
    active = rng.uniform(size=mat.shape) >= 0.1
    isb = np.zeros(T, np.uint8)
    isb[np.argsort(rng.normal(size=T), kind="stable")[:N_BELOW]] = 1
    return mat, active, isb, p


# ---------------------------------------------------------------------------
# b. mixed K in one launch
# ---------------------------------------------------------------------------
LEVELS = {"kr4": (2, 3, 4), "kr8": (3, 5, 8), "kr16": (4, 9, 16, 17),
          "all": (2, 3, 8, 16, 17, 40, 256, 257, 300)}
N_MIXED = (1001, TILE * 16 + 3)     # next to each other in a launch
BASE_MIXED = (0, 3)
N_PREFIXED = 1 << 17                # every job's n_cand in the prefix-first runs
MIXED_ABOVE = 400


def variant(ks):
    """launch_cat's KR for a launch of these category counts."""
    return next((kr for kr in KR if max(ks) <= kr), KR[-1])


def regime(K, kr):
    return "regs" if K <= kr else ("search" if K <= K_KEY else "plain")


@functools.lru_cache(maxsize=None)
def level(name):
    jobs, lv = [], sorted(LEVELS).index(name)
    for j, K in enumerate(LEVELS[name]):
        rng = np.random.RandomState(7000 + 1000 * lv + K)
        jobs.append(Job("%s:randint(%d)" % (name, K), "randint", (K,), rng.randint(0, K, N_BELOW),
                        rng.randint(0, K, MIXED_ABOVE), _key(100 * lv + j),
                        N_MIXED[j % 2], BASE_MIXED[(j >> 1) % 2]))
    return tuple(jobs)


# ---------------------------------------------------------------------------
# c. tied best categories
# ---------------------------------------------------------------------------
TIE_K, TIE_CATS, TIE_T = 8, (0, 5), 10_000
TIE_KEYS = tuple(_key(1000 + i) for i in range(8))
TIE_N = (1001, 1 << 17)


def tie_history(seed=1):
    rng = np.random.RandomState(seed)
    above = rng.choice([1, 2, 3, 4, 6, 7], size=TIE_T - N_BELOW)
    below = rng.choice([1, 2], size=N_BELOW)
    return below, above


def tie_jobs(n_cand, seed=1):
    below, above = tie_history(seed)
    return tuple(Job("tie:%d" % i, "randint", (TIE_K,), below, above, key, n_cand, 0)
                 for i, key in enumerate(TIE_KEYS))


# ---------------------------------------------------------------------------
# d. zero prior probabilities
# ---------------------------------------------------------------------------
ZERO_P = (0.3, 0.0, 0.3, 0.0, 0.4, 0.0)
ZERO_BELOW = (0, 2, 3, 3, 4, 0, 2)
ZERO_NAN, ZERO_PINF, ZERO_NINF = 1, 3, 5
ZERO_INJ = (0, 2, 4, 3, 5, 3, 1, 0, 1)
ZERO_KEYS = tuple(_key(2000 + i) for i in range(4))


def zero_job(key=ZERO_KEYS[0], n_cand=1001, cand_base=0, seed=2, last_nan=False):
    """last_nan: category 5 observed on neither side, so the LAST category
    scores NaN too -- better than any winner, and without a word of its own
    (before the saturated-threshold rule it held the word 2^32 - 1, and kept
    every prefix-first decision open)."""
    above = np.random.RandomState(seed).choice([0, 2, 4] if last_nan else [0, 2, 4, 5], size=400)
    return Job("zero/last" if last_nan else "zero", "categorical", (ZERO_P,),
               np.array(ZERO_BELOW), above, key, n_cand, cand_base)


# ---------------------------------------------------------------------------
# e. rare tied best categories
# ---------------------------------------------------------------------------
RARE_N = 1 << 20
RARE_TINY = 1.03e-3      # below mass 6 p / 31 = 1.99e-4
RARE_P = (0.25, 0.25, 0.25, 0.25 - 2 * RARE_TINY, RARE_TINY, RARE_TINY)
RARE_CATS = (4, 5)
RARE_KEYS = tuple(_key(3000 + i) for i in range(16))


def rare_jobs(n_cand=RARE_N, seed=3):
    rng = np.random.RandomState(seed)
    below, above = rng.choice(4, size=N_BELOW), rng.choice(4, size=TIE_T - N_BELOW)
    return tuple(Job("rare:%d" % i, "categorical", (RARE_P,), below, above, key, n_cand, 0)
                 for i, key in enumerate(RARE_KEYS))


def situation(kp, cats=RARE_CATS):
    """How many of the tied categories the draws kp hold: 0, 1 or 2."""
    return int(sum(bool(np.any(kp == c)) for c in cats))


# ---------------------------------------------------------------------------
# the replay of one job
# ---------------------------------------------------------------------------
def job_posteriors(job, pw=1.0, lf=O.DEFAULT_LF):
    return tuple(posterior(job.kind, job.args, o, pw, lf) for o in (job.below, job.above))


def scores(pb, pa):
    """log p_below - log p_above per category (categorical_lpdf, tpe.py:60-73)."""
    with np.errstate(all="ignore"):
        return np.log(pb) - np.log(pa)


def job_scores(job):
    return scores(*job_posteriors(job))


def oracle_cdf(job):
    """The cumulative below p the CPU premises replay on (the device's own,
    within K 2^-52 of it, is what the GPU tests replay on)."""
    return np.cumsum(job_posteriors(job)[0])


def intervals(cdf):
    """(lo, hi): category k takes the words [lo[k], hi[k]) -- thr[k-1] to
    thr[k], the first category counting from 0 and the last one with mass up
    to 2^32 (a saturated threshold counts as 2^32, so a trailing category of
    probability zero takes no word: oracle.streams.categorical_intervals)."""
    return S.categorical_intervals(cdf)


def draw(cdf, key, cand_base, n):
    return S.categorical_draw(cdf, key, cand_base + np.arange(n, dtype=np.int64))


def first_of(cdf, key, cand_base, n, cats, chunk=1 << 14):
    """Local index of the first candidate that holds one of `cats` (-1: none),
    scanning the stream chunk by chunk."""
    for a in range(0, n, chunk):
        k = draw(cdf, key, cand_base + a, min(chunk, n - a))
        hit = np.flatnonzero(np.isin(k, cats))
        if hit.size:
            return a + int(hit[0])
    return -1


def maximal(score):
    """Categories np.argmax could return were they all drawn: the NaN ones if
    any, else those of the largest score."""
    nan = np.isnan(score)
    return nan if nan.any() else score == score.max()


def need_flag(kp, score, cdf, n_cand, prefix=PREFIX):
    """The prefix-first decision after the first `prefix` candidates kp: the
    rest of the stream is needed when it exists, no category of maximal score
    occurs in the prefix, and some category scoring strictly better than the
    prefix's winner (np.argmax's order: NaN first) has a non-empty interval."""
    if n_cand <= prefix:
        return 0
    if maximal(score)[kp].any():
        return 0
    sp = score[kp]
    w = sp[np.argmax(sp)]
    better = np.zeros(score.size, bool) if np.isnan(w) else (np.isnan(score) | (score > w))
    lo, hi = intervals(cdf)
    return int(np.any(better & (hi > lo)))


def replay(job, cdf, score=None, prefix=PREFIX):
    """One job's expected outcome on the cumulative p `cdf`: dict with the
    stream `k`, np.argmax's `index` (global), `value`, `score`, and `need`."""
    score = job_scores(job) if score is None else score
    k = draw(cdf, job.key, job.cand_base, job.n_cand)
    s = score[k]
    win = int(np.argmax(s))
    return dict(k=k, index=job.cand_base + win, value=int(k[win]), score=s[win],
                need=need_flag(k[:prefix], score, cdf, job.n_cand, prefix))
