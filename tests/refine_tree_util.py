"""Cases the CPU and the GPU tests of ``refine_tree=`` share (joint.py,
"Refining in a tree")."""
import numpy as np

from hyperopt_amd import Domain, hp, rand, tpe
from hyperopt_amd import joint as J
from tests import joint_util as U
from tests.refine_util import KW


def tree_case(space, configs, losses, P, seed, force=None):
    """(domain, trials, hist, rows' values): the given history and P random rows
    (``force``: {label: value} every row holds), NaN where a label is not live."""
    domain = Domain(lambda x: 0, space)
    labels = list(domain.params)
    trials = U.make_trials(domain, configs, np.asarray(losses, float))
    rng = np.random.RandomState(seed)
    rows = []
    while len(rows) < P:
        c = rand.sample_config(domain, rng)
        if all(c.get(k) == v for k, v in (force or {}).items()):
            rows.append(c)
    vals = np.asarray([[float(c.get(lab, np.nan)) for lab in labels] for c in rows])
    return domain, trials, tpe.collect_history(trials, labels), vals.reshape(P, len(labels))


def random_tree_case(space, T, P, seed, loss=None, force=None):
    """``tree_case`` on T random trials (uniform losses, or ``loss(config)``)."""
    domain = Domain(lambda x: 0, space)
    rng = np.random.RandomState(seed)
    configs = [rand.sample_config(domain, rng) for _ in range(T)]
    losses = [rng.uniform() if loss is None else loss(c) for c in configs]
    return tree_case(space, configs, losses, P, seed + 1, force)


def kinds_space():
    """Root: two continuous labels and a 3-way choice.  Branch A: uniform,
    loguniform, quniform and a nested choice one option of which holds a normal
    and a lognormal; branch B: a randint alone (D_c = 0); branch C: empty."""
    nested = hp.choice("n", [{"an": hp.normal("an", 0, 1), "aln": hp.lognormal("aln", 0, 1)},
                             {}])
    return {"x": hp.uniform("x", -1, 2), "y": hp.normal("y", 0, 1),
            "s": hp.choice("s", [{"au": hp.uniform("au", 0, 1),
                                  "alu": hp.loguniform("alu", -3, 0),
                                  "aq": hp.quniform("aq", 0, 6, 2), "n": nested},
                                 {"br": hp.randint("br", 4)}, {}])}


def safe_tree_rows(domain, hist, cand, refine, n, kw=KW):
    """``refine_util.safe_rows``' rule per group: the first n rows of ``cand``
    every decision of which, in every live group, has |J(t') - J(t)| >= 100 x
    the bound in the reference alone -- found among the first 4 n candidates."""
    margin = J.refine_tree_numpy(domain, hist, cand[:4 * n], refine, return_info=True,
                                 **kw)[5]["margin"]
    safe = np.flatnonzero(~(margin < 100.0).any((0, 2)))
    assert safe.size >= n, (safe.size, n)
    return cand[safe[:n]]
