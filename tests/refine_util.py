"""Cases the CPU and the GPU tests of ``refine=`` share (joint.py, "Refining")."""
import functools

import numpy as np

from hyperopt_amd import Domain, hp, rand, tpe
from hyperopt_amd import joint as J
from tests import joint_util as U

KW = dict(prior_weight=0.7, gamma=0.3, bandwidth=0.25, cat_smoothing=0.5)


def random_case(space, T, P, seed, loss=None):
    """(domain, trials, hist, rows' values): T random trials, P random rows."""
    domain = Domain(lambda x: 0, space)
    labels = list(domain.params)
    rng = np.random.RandomState(seed)
    configs = [rand.sample_config(domain, rng) for _ in range(T)]
    losses = np.asarray([rng.uniform() if loss is None else loss(c) for c in configs])
    if T > 11:
        losses[11] = np.inf  # a failed trial sits above
    trials = U.make_trials(domain, configs, losses)
    rows = [rand.sample_config(domain, rng) for _ in range(P)]
    vals = np.asarray([[float(c[lab]) for lab in labels] for c in rows]).reshape(P, len(labels))
    return domain, trials, tpe.collect_history(trials, labels), vals


@functools.lru_cache(None)
def all_kinds_case(P=24):
    """The all-kinds case: 80 trials, P rows, rows 5 and 9 with J = NaN (a
    qnormal far tail; the pchoice option of probability zero); built once."""
    case = random_case(U.all_kinds_space(hp), 80, P, 5)
    labels = list(case[0].params)
    case[3][5, labels.index("i")], case[3][9, labels.index("k")] = 2.0e6, 0.0
    return case


def safe_rows(domain, hist, cand, refine, n, kw=KW):
    """The first n rows of ``cand`` every decision of which has, in the reference
    alone, |J(t') - J(t)| >= 100 x the bound (no decision, or t' == t: no miss)."""
    margin = J.refine_numpy(domain, hist, cand, refine, return_info=True, **kw)[5]["margin"]
    safe = np.flatnonzero(~(margin < 100.0).any(0))
    assert safe.size >= n, (safe.size, n)
    return cand[safe[:n]]
