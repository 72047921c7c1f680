"""The liar batch (hyperopt_amd/joint.py, "Batches") restated with scalar
loops, for the tests.

One Python loop per index, on tests/joint_util.py's factor functions, and
independent of ``joint.liar_numpy``: only the history and its split come from
the package, as in joint_util.  Everything is a Python float (fp64).
"""
import math

import numpy as np

from hyperopt_amd import tpe
from oracle import tpe_oracle as O
from tests import joint_util as U

NEG_INF = U.NEG_INF


def first_row(S, gone):
    """The first row of S outside ``gone``: larger first, NaN before
    everything, equal scores (-0.0 == +0.0) to the smaller row; -1: none."""
    best = -1
    for r in range(len(S)):
        if gone[r]:
            continue
        if S[r] != S[r]:
            return r  # (the first NaN in row order)
        if best < 0 or S[r] > S[best]:
            best = r
    return best


def gap_to_runner_up(S, gone, p, X):
    """S[p] minus the best score of the other free rows that do not hold row
    p's values (exact twins excepted); +inf where there is none, NaN where the
    pick's score is NaN."""
    if S[p] != S[p]:
        return float("nan")
    other = [S[r] for r in range(len(S)) if r != p and not gone[r] and X[r] != X[p]]
    return S[p] - max(other) if other else float("inf")


def lie_component(infos, X, p, sigma):
    """Row p as a trial component, per label: (is prior, mu or category,
    sigma, log Z) as ``joint_util.factor`` takes it."""
    comp = []
    for d, info in enumerate(infos):
        if info["cls"] == "cat":
            comp.append((False, int(round(X[p][d])) - info["low"], 0.0, 0.0))
        else:
            mu = U.fit(info, X[p][d])
            comp.append((False, mu, sigma[d], U.log_z(info, mu, sigma[d])))
    return comp


def lie_picks(infos, X, S0, A0, sigma, log_w, log_lie, a, k, gone=None, forced=None):
    """The definition, loop by loop.  ``X``: P rows of D stored values (lists);
    ``S0`` / ``A0``: P floats; ``sigma``: D bandwidths; ``a``: cat_smoothing;
    ``gone``: P flags (taken, or masked by ``distinct``).  Returns a dict:
    rows, S_at_pick, S_k, U_0, U_k, and per pick the gap to the runner-up.

    ``forced``: a pick sequence to follow in place of the definition's own (a
    device's, whose scores differ from these in their last bits): ``regret``
    then holds, per pick, the score of the definition's choice minus the score
    of the forced one -- 0.0 where they are the same row, exact twins, or both
    scores are NaN; +inf where the forced row was not free, or a NaN row was
    passed over."""
    P = len(X)
    gone = [False] * P if gone is None else [bool(g) for g in gone]
    U0 = [log_w + float(A0[r]) for r in range(P)]
    Uc, S = list(U0), [float(s) for s in S0]
    rows, at, gaps, regret = [], [], [], []
    for j in range(min(max(int(k), 0), P)):
        p = first_row(S, gone)
        if p < 0:
            break
        if forced is not None:
            if j >= len(forced):
                break
            f = int(forced[j])
            if f != p:
                if not 0 <= f < P or gone[f] or S[p] != S[p]:
                    regret.append(float("inf"))
                    break
                regret.append(S[p] - S[f])
                p = f
            else:
                regret.append(0.0)
        gaps.append(gap_to_runner_up(S, gone, p, X))
        rows.append(p)
        at.append(S[p])
        gone[p] = True
        comp = lie_component(infos, X, p, sigma)
        for r in range(P):
            c = log_lie
            for d, info in enumerate(infos):
                c = c + U.factor(info, X[r][d], comp[d], a)
            if c != NEG_INF:
                m = c if c > Uc[r] else Uc[r]
                Uc[r] = NEG_INF if m == NEG_INF else \
                    m + math.log(math.exp(Uc[r] - m) + math.exp(c - m))
            S[r] = float(S0[r]) - (Uc[r] - U0[r]) if math.isfinite(U0[r]) else float(S0[r])
    return dict(rows=rows, S_at_pick=np.asarray(at, np.float64), S_k=np.asarray(S, np.float64),
                U_0=np.asarray(U0), U_k=np.asarray(Uc), gaps=np.asarray(gaps, np.float64),
                regret=np.asarray(regret, np.float64))


def above_set(domain, trials, gamma, lf, prior_weight, bandwidth):
    """(infos, cols, sigma, log W) of the lie under the above set of
    ``trials``: n its rows with every joint label active, sigma the set's
    bandwidths (a set of one row's where n == 0), W the sum of its ramp and
    the prior's weight."""
    labels = list(domain.params)
    names = U.joint_label_names(domain)
    cols = [labels.index(lab) for lab in names]
    infos = [U.label_info(domain.specs[lab]) for lab in names]
    hist = tpe.collect_history(trials, labels)
    n = 0
    if hist.tids.size:
        isa = tpe.split_masks(hist, gamma)[1]
        n = sum(1 for r in range(hist.tids.size)
                if isa[r] and all(hist.active[r, j] for j in cols))
    D = len(cols)
    sigma = [bandwidth * info["sigma"] * float(max(n, 1)) ** (-1.0 / (D + 4)) for info in infos]
    total = sum(float(w) for w in O.linear_forgetting_weights(n, lf)) + float(prior_weight)
    return infos, cols, sigma, math.log(total)


def liar_reference(domain, trials, vals, S0, A0, k, gone=None, lie_weight=1.0, prior_weight=1.0,
                   gamma=0.25, lf=25, bandwidth=0.2, cat_smoothing=1.0):
    """``lie_picks`` of the rows ``vals`` ((P, L) stored values in
    ``domain.params`` column order) under the above set of ``trials``."""
    infos, cols, sigma, log_w = above_set(domain, trials, gamma, lf, prior_weight, bandwidth)
    X = [[float(vals[r, j]) for j in cols] for r in range(vals.shape[0])]
    return lie_picks(infos, X, S0, A0, sigma, log_w, math.log(lie_weight), float(cat_smoothing),
                     k, gone)
