"""Case table shared by tests/test_settings_cases.py (the oracle alone, no GPU)
and tests/test_gpu_settings.py (the kernels): TPE's own settings away from
their defaults -- linear forgetting LF != 25, prior weight != 1, and below
sets long enough to carry a ramp (LF < 25, so n_below > LF).

A case is (lf, prior_weight, n_below, n_above, inactive share, seed) plus the
group it belongs to; the counts are history rows (the lists of a label are
the active ones among them), or list lengths for the upload groups:

  fit     a DeviceHistory of T = n_below + n_above rows over the space of
          tests/test_gpu_sorted_fit.py, fitted from the resident history by
          both fits (tpe_fit_sorted / tpe_gather_obs + tpe_parzen_fit).
          Column 0 is active in every row, the others lose `inactive` of
          theirs, so at LF = 24 the 25 below rows of column 0 carry a ramp of
          ONE entry (LfRamp's num == 1 branch) and no other column has one
  count   categorical and randint(low != 0) counts: `up` uploaded lists
          (k_cat_counts), `hist` a history of T rows (k_cat_counts_hist below
          32 768 rows, the chunked k_cath_* from there on); `pin`: the lists of
          (LF, n) = (1, 15) and (2, 10) whose observation at ramp position
          num - 1 is alone in its category
  score   one label of one kind, 2048 injected candidates, histories of 30
          and 3000 points (min(n, 25) of them below)

The reference never passes linear_forgetting on from tpe.suggest, so these
cases have no end-to-end reference run; the oracle (pinned to the reference's
unit functions at these settings by tests/golden/units_settings.npz) is the
yardstick.  parzen() / cat_post() give the oracle's arrays under one of three
seeded slips, which tests/test_settings_cases.py shows this table can tell apart.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import tpe_oracle as O
from tests.test_gpu_parity import KINDS
from tests.test_gpu_sorted_fit import SPACE, _cols

Case = namedtuple("Case", "name group lf pw n_below n_above inactive seed tags kind args")

N_INJ = 2048
P_CAT = (0.1, 0.2, 0.3, 0.15, 0.25)   # K*(pw*p) != (K*pw)*p at pw = 0.3 and 1e-3
RANDINT = (3, 9)
PINS = ((1, 15), (2, 10))             # fl((num-1)*step + start) != 1.0: the pin matters
FIT_LF = (1, 7, 24)
FIT_T = (26, 1023, 1024, 1025, 2049, 5000)   # 1024: kChunk of tpe_sorted.hip
FIT_PW = (0.3, 7.5, 1e-3)
COUNT_LF = (1, 2, 7, 26)
COUNT_PW = (0.3, 1e-3)
COUNT_T = (7680, 7681, 32769)         # the kCHW window, one row more, the chunked walk
SCORE_SETTINGS = ((0.3, 7), (7.5, 1))
SCORE_N = (30, 3000)
SCORE_KINDS = list(KINDS) + [("randint", RANDINT), ("categorical", (P_CAT,))]
# seeds of the scoring cases that were moved off a near tie of the two best
# candidates (tests/test_settings_cases.py test_scoring_margins); default: 0
SCORE_SEEDS = {"score uniform pw=0.3 lf=7 n=30": 6, "score uniform pw=7.5 lf=1 n=30": 2,
               "score uniform pw=7.5 lf=1 n=3000": 1, "score loguniform pw=0.3 lf=7 n=30": 15,
               "score loguniform pw=7.5 lf=1 n=30": 14, "score lognormal pw=7.5 lf=1 n=30": 2}


def _build():
    cases = []

    def add(name, group, lf, pw, nb, na, inactive, seed, tags=(), kind=None, args=None):
        cases.append(Case(name, group, lf, pw, nb, na, inactive, seed, frozenset(tags), kind,
                          args))

    for i, lf in enumerate(FIT_LF):
        for k, T in enumerate(FIT_T):
            nb = min(25, T - 1)
            add("fit lf=%d T=%d" % (lf, T), "fit", lf, FIT_PW[(i + k) % 3], nb, T - nb, 0.3,
                8000 + 100 * i + k, ["below-ramp"])
    d = 0
    for lf in COUNT_LF:
        for pw in COUNT_PW:
            # below: n - lf in 1, 2, 3, 0 in turn; above: one case per lf past
            # one k_cat_counts step (1024 observations)
            nb = lf + (1, 2, 3, 0)[d % 4]
            add("up lf=%d pw=%g" % (lf, pw), "count_up", lf, pw, nb, 1025 if pw == 0.3 else 40,
                0.0, 8300 + d, ["below-ramp"] if nb > lf else [])
            d += 1
    for lf, n in PINS:
        for pw in COUNT_PW:
            add("pin lf=%d n=%d pw=%g" % (lf, n, pw), "count_up", lf, pw, n, n, 0.0, 8400 + lf,
                ["below-ramp", "pin"])
    for T in COUNT_T:
        for lf in COUNT_LF:
            for pw in COUNT_PW:
                add("hist T=%d lf=%d pw=%g" % (T, lf, pw), "count_hist", lf, pw, 25, T - 25, 0.15,
                    8500 + T % 97, ["below-ramp"] if lf < 20 else [])
    for kind, args in SCORE_KINDS:
        for pw, lf in SCORE_SETTINGS:
            for n in SCORE_N:
                name = "score %s pw=%g lf=%d n=%d" % (kind, pw, lf, n)
                add(name, "score", lf, pw, min(n, 25), n, 0.0, SCORE_SEEDS.get(name, 0),
                    ["below-ramp"], kind, args)
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
_INDEX = {c.name: i for i, c in enumerate(CASES)}
assert len(BY_NAME) == len(CASES)


def group(g):
    return [c for c in CASES if c.group == g]


# ---------------------------------------------------------------------------
# the oracle, restated with one slip at a time
# ---------------------------------------------------------------------------
def ramp_at(pos, n, lf, pinned=True):
    """LfRamp::at (tpe_common.hpp) == linear_forgetting_weights(n, lf)[pos];
    pos >= n - lf gives 1 (a row index used for a rank lands there).
    ``pinned=False``: slip (a), the last ramp entry computed like the others."""
    pos = np.asarray(pos, np.int64)
    num = n - lf
    if not (0 < lf < n):
        return np.ones(pos.shape)
    if num == 1:
        return np.where(pos >= num, 1.0, 1.0 / n)
    start = 1.0 / n
    step = (1.0 - start) / (num - 1)
    w = pos * step + start
    if pinned:
        w = np.where(pos == num - 1, 1.0, w)
    return np.where(pos >= num, 1.0, w)


def _weights(n, lf, slip, rows):
    pos = np.arange(n) if (slip != "b" or rows is None) else np.asarray(rows)
    return ramp_at(pos, n, lf, pinned=slip != "a")


def parzen(obs, pw, pmu, psig, lf, slip=None, rows=None):
    """O.adaptive_parzen_normal with the ramp of ``slip``: None (the oracle's
    own bits, asserted by the CPU test), "a" (endpoint not pinned), "b" (the
    ramp indexed by the member's history row ``rows``, not its rank)."""
    w0, mu, sig = O.adaptive_parzen_normal(obs, pw, pmu, psig, lf)
    n = np.size(obs)
    if not (lf and lf < n):
        return w0, mu, sig
    order = np.argsort(np.asarray(obs, float), kind="stable")
    pos = int(np.searchsorted(np.asarray(obs, float)[order], pmu))
    w = np.insert(_weights(n, lf, slip, rows)[order], pos, pw)
    return w / w.sum(), mu, sig


def cat_post(kind, obs, pw, lf, slip=None, rows=None):
    """O.categorical_posterior / O.randint_posterior of the table's two label
    kinds under ``slip`` ("c": (K*pw)*p in place of K*(pw*p))."""
    obs = np.asarray(obs, np.int64)
    n = obs.size
    p = np.asarray(P_CAT)
    K, off = (p.size, 0) if kind == "categorical" else (RANDINT[1] - RANDINT[0], RANDINT[0])
    wts = _weights(n, lf, slip, rows) if n else None
    counts = np.bincount(obs - off, wts, K)
    if kind == "randint":
        pseudo = counts + pw
    elif slip == "c":
        pseudo = counts + (K * pw) * p
    else:
        pseudo = counts + K * (pw * p)
    return pseudo / np.sum(pseudo)


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def split_rows(losses, n_below):
    isb = np.zeros(losses.size, np.uint8)
    isb[np.argsort(losses, kind="stable")[:n_below]] = 1
    return isb


@functools.lru_cache(maxsize=None)
def fit_history(name):
    """(mat, active, losses, is_below) of a fit case: _cols' eight columns."""
    c = BY_NAME[name]
    T = c.n_below + c.n_above
    rng = np.random.RandomState(c.seed)
    mat = _cols(T, rng)
    active = rng.uniform(size=mat.shape) >= c.inactive
    active[:, 0] = True
    losses = rng.normal(size=T)
    return mat, active, losses, split_rows(losses, c.n_below)


def fit_lists(name, j):
    """Column j's (below, above) observations and their history rows, tid order."""
    mat, active, _, isb = fit_history(name)
    out = []
    for side in (1, 0):
        rows = np.flatnonzero(active[:, j] & (isb == side))
        out.append((mat[rows, j], rows))
    return out


def fit_expected(name, j, slip=None, lf=None):
    """Column j's two posteriors: (w, mu, sigma) twice, or (p_below, p_above)
    for the randint column."""
    c = BY_NAME[name]
    lf = c.lf if lf is None else lf
    lab, kind, args = SPACE[j]
    lists = fit_lists(name, j)
    if kind == "randint":
        return tuple(_randint6(obs, c.pw, lf, slip, rows) for obs, rows in lists)
    fam, pmu, psig, tf, _, _, _ = O.posterior_spec(kind, args)
    return tuple(parzen(tf(obs), c.pw, pmu, psig, lf, slip, rows) for obs, rows in lists)


def _randint6(obs, pw, lf, slip, rows):  # SPACE's randint(6)
    wts = _weights(obs.size, lf, slip, rows) if obs.size else None
    pseudo = np.bincount(obs.astype(np.int64), wts, 6) + pw
    return pseudo / np.sum(pseudo)


def _alone(rng, n, lf, K):
    obs = rng.randint(0, K - 1, n)
    obs[n - lf - 1] = K - 1
    return obs


@functools.lru_cache(maxsize=None)
def count_lists(name):
    """An upload count case: category ids (below, above), shared by both label
    kinds (randint adds its `low`)."""
    c = BY_NAME[name]
    rng = np.random.RandomState(c.seed)
    K = len(P_CAT)
    if "pin" in c.tags:
        return _alone(rng, c.n_below, c.lf, K), _alone(rng, c.n_above, c.lf, K)
    return rng.randint(0, K, c.n_below), rng.randint(0, K, c.n_above)


@functools.lru_cache(maxsize=None)
def count_history(T):
    """(mat, active, is_below) of the count_hist cases of T rows: column 0 the
    categorical label, column 1 randint (stored with its `low`)."""
    c = next(c for c in group("count_hist") if c.n_below + c.n_above == T)
    rng = np.random.RandomState(c.seed)
    K = len(P_CAT)
    mat = np.stack([rng.choice(K, size=T, p=P_CAT).astype(float),
                    rng.randint(RANDINT[0], RANDINT[1], T).astype(float)], axis=1)
    active = rng.uniform(size=mat.shape) >= c.inactive
    return mat, active, split_rows(rng.normal(size=T), c.n_below)


def count_hist_lists(T, j):
    mat, active, isb = count_history(T)
    out = []
    for side in (1, 0):
        rows = np.flatnonzero(active[:, j] & (isb == side))
        out.append((mat[rows, j].astype(np.int64), rows))
    return out


def count_expected(c, slip=None, lf=None):
    """{kind: (p_below, p_above)} of a count case."""
    lf = c.lf if lf is None else lf
    out = {}
    for j, kind in enumerate(("categorical", "randint")):
        if c.group == "count_up":
            off = RANDINT[0] if kind == "randint" else 0
            lists = [(o + off, None) for o in count_lists(c.name)]
        else:
            lists = count_hist_lists(c.n_below + c.n_above, j)
        out[kind] = tuple(cat_post(kind, o, c.pw, lf, slip, rows) for o, rows in lists)
    return out


@functools.lru_cache(maxsize=None)
def score_inputs(name):
    """(obs_below, obs_above, candidates) of a scoring case."""
    c = BY_NAME[name]
    rng = np.random.RandomState(9000 + 1000 * c.seed + _INDEX[name])
    kind, a = c.kind, c.args
    if kind == "randint":
        draw = lambda n: rng.randint(a[0], a[1], n)  # noqa: E731
    elif kind == "categorical":
        draw = lambda n: rng.choice(len(a[0]), size=n, p=a[0])  # noqa: E731
    elif kind in ("uniform", "quniform"):
        draw = lambda n: rng.uniform(a[0], a[1], n)  # noqa: E731
    elif kind in ("loguniform", "qloguniform"):
        draw = lambda n: np.exp(rng.uniform(a[0], a[1], n))  # noqa: E731
    elif kind in ("normal", "qnormal"):
        draw = lambda n: rng.normal(a[0], a[1], n)  # noqa: E731
    else:
        draw = lambda n: np.exp(rng.normal(a[0], a[1], n))  # noqa: E731
    out = [draw(c.n_below), draw(c.n_above), draw(N_INJ)]
    if kind == "randint":  # injected categorical candidates are category ids (tpe.py:590)
        out[2] = out[2] - a[0]
    if kind in O.CONTINUOUS and kind.startswith("q"):
        out = [np.round(v / a[2]) * a[2] for v in out]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def score_expected(name):
    """The oracle's result dict of a scoring case (computed once, shared)."""
    c = BY_NAME[name]
    below, above, cand = score_inputs(name)
    with np.errstate(all="ignore"):
        if c.kind in O.CONTINUOUS:
            return O.continuous_label_scores(c.kind, c.args, below, above, cand, c.pw, c.lf)
        return O.categorical_label_scores(c.kind, c.args, below, above, cand, c.pw, c.lf)


def margin(name):
    """(best score, its lead over the best candidate of another value).  Equal
    candidates (quantized and categorical kinds repeat values) score alike on
    any implementation, and the first of them wins."""
    ref = score_expected(name)
    cand = np.asarray(score_inputs(name)[2], float)
    s = ref["below_llik"] - ref["above_llik"]
    best = s[ref["best"]]
    other = s[cand != cand[ref["best"]]]
    return float(best), float(best - other.max())
