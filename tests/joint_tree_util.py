"""The joint criterion per group of labels (``joint="tree"``) restated with
scalar loops, for the tests.

Written from the model's definition (hyperopt_amd/joint.py's module text,
"Groups") and independent of ``hyperopt_amd/joint.py``: the
groups are read off ``domain.live_program()`` here, a set is built by
``tests/joint_util.py``'s ``set_components`` (which drops the rows that lack
one of the group's labels and takes D from the group) and a row is scored by
its ``log_l``.  Only the history and its split come from the package.

The cases the CPU and the GPU tests share are at the end.
"""
import numpy as np

from hyperopt_amd import Domain, hp, rand, tpe
from tests import joint_util as U


def groups_of(domain):
    """[(clauses, labels)]: labels with identical clause tuples, in
    ``domain.params`` order, groups by their first label."""
    prog = domain.live_program()
    out = []
    for lab in domain.params:
        for clauses, labs in out:
            if clauses == prog[lab]:
                labs.append(lab)
                break
        else:
            out.append((prog[lab], [lab]))
    return out


def tree_reference(domain, trials, vals, active, prior_weight=1.0, gamma=0.25, lf=25,
                   bandwidth=0.2, cat_smoothing=1.0):
    """(S, J, log L_below, log L_above, [(n_below, n_above)]) of the rows
    ``vals`` ((P, L) stored values) with activity ``active``: S (P,), the rest
    (P, G), NaN where the group is not live in the row."""
    labels = list(domain.params)
    groups = groups_of(domain)
    hist = tpe.collect_history(trials, labels)
    isb, isa = tpe.split_masks(hist, gamma) if hist.tids.size else ([], [])
    P, G = vals.shape[0], len(groups)
    J, LB, LA = (np.full((P, G), np.nan) for _ in range(3))
    ns = []
    for g, (_clauses, labs) in enumerate(groups):
        cols = [labels.index(lab) for lab in labs]
        infos = [U.label_info(domain.specs[lab]) for lab in labs]
        sets = [U.set_components(infos, cols, hist, mask, lf, prior_weight, bandwidth)
                for mask in (isb, isa)]
        ns.append((sets[0][2], sets[1][2]))
        for r in range(P):
            if not all(active[r, j] for j in cols):
                continue
            x = [float(vals[r, j]) for j in cols]
            LB[r, g], LA[r, g] = (U.log_l(infos, logw, comps, x, float(cat_smoothing))
                                  for logw, comps, _n in sets)
            with np.errstate(invalid="ignore"):
                J[r, g] = LB[r, g] - LA[r, g]
    return fold_live(J, group_live(domain, np.asarray(active, bool))), J, LB, LA, ns


def fold_live(J, live):
    """S from the (P, G) matrix of J_g and the groups' liveness ((P, G) bool):
    column 0 (the root group, live in every row) assigned, then the live
    columns added in order."""
    S = J[:, 0].copy()
    for g in range(1, J.shape[1]):
        with np.errstate(invalid="ignore"):
            S = np.where(live[:, g], S + J[:, g], S)
    return S


def group_live(domain, active):
    """(P, G) bool: group g is live in row r (its first label is)."""
    labels = list(domain.params)
    return np.stack([active[:, labels.index(labs[0])] for _c, labs in groups_of(domain)], 1)


def tolerance(LB, LA):
    """1e-6 * sum over the live groups of |log L_below,g| + |log L_above,g|."""
    return 1e-6 * (np.nansum(np.abs(LB), 1) + np.nansum(np.abs(LA), 1))


# -- the cases -------------------------------------------------------------------
def nested_case():
    """(domain, trials, pool, kw) of the suite's ``nested`` case with 300
    sampled rows, as tests/test_gpu_joint.py builds them."""
    from tests.test_gpu_pool import _case
    _arrays, meta, trials, domain = _case("nested")
    rng = np.random.RandomState(11)
    pool = tpe.Pool(domain, [rand.sample_config(domain, rng) for _ in range(300)])
    return domain, trials, pool, dict(prior_weight=meta["prior_weight"], gamma=meta["gamma"])


def two_clause_space():
    """``w`` is reachable from two branches of ``s`` (two clauses); ``x`` and
    ``y`` share one clause; ``z`` sits two levels down."""
    w = hp.uniform("w", 0, 1)
    inner = hp.choice("t", [{"z": hp.normal("z", 0, 1)}, {"zz": hp.randint("zz", 3)}])
    first = {"w": w, "x": hp.uniform("x", 0, 1), "y": hp.quniform("y", 0, 8, 2)}
    return {"s": hp.choice("s", [first, {"w": w, "inner": inner},
                                 {"lone": hp.lognormal("lone", 0, 1)}]),
            "free": hp.uniform("free", -1, 1)}


def branch_space():
    """The conditional diagonal case's space: the two interacting choices
    under branch 0 of ``v``, a uniform under branch 1."""
    return {"v": hp.choice("v", [{"a": hp.choice("a", [0, 1, 2, 3]),
                                  "b": hp.choice("b", [0, 1, 2, 3])},
                                 {"c": hp.uniform("c", 0, 1)}])}


GAMMA_DIAGONAL = 1.6  # min(ceil(1.6 sqrt(100)), 25) = 16 below rows: the diagonal trials


def branch_diagonal_case():
    """(domain, trials): 64 trials of branch 0 -- every (a, b) cell four times
    in ``joint_util.diagonal_case``'s order, loss [a != b] + 1e-6 tid -- then
    36 trials of branch 1 with loss 2 + 1e-6 tid."""
    _space, configs, _losses = U.diagonal_case(hp)
    domain = Domain(lambda x: 0, branch_space())
    rng = np.random.RandomState(5)
    cfgs = [dict(c, v=0) for c in configs] + [{"v": 1, "c": float(u)} for u in rng.uniform(size=36)]
    losses = [float(c["a"] != c["b"]) + 1e-6 * tid if c["v"] == 0 else 2.0 + 1e-6 * tid
              for tid, c in enumerate(cfgs)]
    return domain, U.make_trials(domain, cfgs, losses)


def branch_pool_rows():
    """The 16 configurations of branch 0 in row order 4 a + b, then one row of
    branch 1."""
    return [dict(r, v=0) for r in U.diagonal_pool_rows()] + [{"v": 1, "c": 0.5}]


def edge_histories():
    """{name: (configs, losses)} on ``branch_space``: a branch never tried
    (the group's sets are empty on both sides), one tried only above, a
    foreign trial with half a group's labels (the best trial: the below side's
    only row, so the group's below set is empty), no trial at all."""
    b1 = [{"v": 1, "c": 0.1 * (i + 1)} for i in range(8)]
    loss = [0.1 * (i + 1) for i in range(8)]
    good_a = [{"v": 0, "a": i % 4, "b": (i + 1) % 4} for i in range(4)]
    return {
        "never_tried": (b1, loss),                               # group (a, b): prior alone twice
        "above_only": (b1 + good_a, loss + [5.0, 6.0, 7.0, 8.0]),    # (a, b): no below row
        "foreign_half": ([{"v": 0, "a": 2}] + good_a + b1, [0.01] + [0.02, 0.5, 0.6, 0.7] + loss),
        "empty": ([], []),
    }
